"""The view sweep's formula (simplenerf_amd/csrc/simplenerf_sweep.h) in numpy, in float32 or float64, with the split sum -- the
views layer's product as g (over the feature vector, once) + u (over the encoded direction, per view) -- exactly as written there;
plus the loaders of tests/golden/view_sweep.npz shared by the host and the GPU tests."""
import json

import numpy
import torch

from oracle import nerf_oracle as oracle
from simplenerf_amd import synth
from tests import util

CASES = ('ndc', 'world')


def encode(d: numpy.ndarray, degree: int) -> numpy.ndarray:
    """[x, sin(2^0 x), cos(2^0 x), ..., sin(2^(L-1) x), cos(2^(L-1) x)] along the last axis, in d's dtype."""
    parts = [d]
    for k in range(degree):
        parts += [numpy.sin(d * d.dtype.type(2.0 ** k)), numpy.cos(d * d.dtype.type(2.0 ** k))]
    return numpy.concatenate(parts, -1)


def view_sweep(w_v, b_v, w_o, b_o, feature, weights, view_dirs, acc=None, white_bkgd=False, dtype=numpy.float64):
    """out (V,n,3).  w_v (Wv, W+3+6L), b_v (Wv), w_o (>=3, Wv), b_o (>=3), feature (n,S,W), weights (n,S), view_dirs (V,n,3),
    acc (n) with white_bkgd.  Every operation runs in ``dtype``."""
    cast = lambda a: numpy.asarray(a).astype(dtype)
    w_v, b_v, w_o, b_o, feature, weights, view_dirs = (cast(a) for a in (w_v, b_v, w_o[:3], b_o[:3], feature, weights, view_dirs))
    width = feature.shape[-1]
    degree = (w_v.shape[1] - width - 3) // 6
    u = b_v + encode(view_dirs, degree) @ w_v[:, width:].T                  # (V,n,Wv)
    g = feature @ w_v[:, :width].T                                          # (n,S,Wv)
    hidden = numpy.maximum(g[None] + u[:, :, None, :], dtype(0))            # (V,n,S,Wv)
    pre = hidden @ w_o.T + b_o
    rgb = dtype(1) / (dtype(1) + numpy.exp(-pre))
    out = (weights[None, :, :, None] * rgb).sum(2, dtype=dtype)
    if white_bkgd:
        out = out + (dtype(1) - cast(acc))[None, :, None]
    return out


def feature_vectors(params: dict, prefix: str, mlp_cfg: dict, points: torch.Tensor) -> torch.Tensor:
    """The views layer's input without the encoded direction, (..., W): the oracle's trunk (oracle.mlp_forward's first half, the
    same calls in the same order) followed by feature_linear, in the dtype of ``params`` and ``points``."""
    F = torch.nn.functional
    lay = oracle.mlp_layout(params, prefix)
    trunk_in = oracle.pos_encode(points.reshape(-1, 3), mlp_cfg['points_positional_encoding_degree'])[:, :lay['pts_in']]
    h = trunk_in
    for i in range(lay['depth']):
        h = F.relu(F.linear(h, params[f'{prefix}pts_linears.{i}.weight'], params[f'{prefix}pts_linears.{i}.bias']))
        if i == oracle.SKIP_AFTER_LAYER:
            h = torch.cat([trunk_in, h], -1)
    feature = F.linear(h, params[f'{prefix}feature_linear.weight'], params[f'{prefix}feature_linear.bias'])
    return feature.reshape(tuple(points.shape[:-1]) + (feature.shape[-1],))


def saved_feature(saved: numpy.ndarray, mlp_cfg: dict, n: int, s: int) -> numpy.ndarray:
    """(n,S,W) feature vectors out of fp32 saved activations: per 32-sample block a [row][32 samples] tile of MlpPlan::act_rows()
    rows, the feature rows from act_feature() on (simplenerf_amd/csrc/mlp_plan.h, restated here)."""
    depth, width, views_width = mlp_cfg['points_net_depth'], mlp_cfg['points_net_width'], mlp_cfg['views_net_width']
    act_feature = 96 + depth * width
    mask_tiles = depth * (width // 32) + views_width // 32
    act_rows = 96 + (depth + 1) * width + views_width + 2 * ((mask_tiles + 1) // 2)
    tiles = numpy.asarray(saved).reshape(-1, act_rows, 32)[:, act_feature:act_feature + width, :]       # (blocks, W, 32)
    return tiles.transpose(0, 2, 1).reshape(-1, width)[:n * s].reshape(n, s, width)


def head_arrays(params: dict, prefix: str):
    """(w_v, b_v, w_o, b_o) of one MLP as numpy arrays."""
    return tuple(params[f'{prefix}{name}'].detach().cpu().numpy() for name in
                 ('views_linears.0.weight', 'views_linears.0.bias', 'views_output_linear.weight', 'views_output_linear.bias'))


_fixture = {}


def load_case(tag: str):
    """-> (arrays of the case without the prefix, model configs of the run (config2 at the scene's ndc / white_bkgd), the scene's
    saved model configs at the 7 x 11 frame, the scene's configs)."""
    if not _fixture:
        _fixture.update(util.load('view_sweep.npz'))
    g = {k[len(tag) + 1:]: v for k, v in _fixture.items() if k.startswith(tag + '_')}
    scene_configs = json.loads(str(g['scene_configs_json']))
    configs = synth.with_overrides(synth.make_configs('config2'), white_bkgd=bool(scene_configs['model']['white_bkgd']))
    configs['data_loader']['ndc'] = bool(scene_configs['data_loader']['ndc'])
    return g, configs, json.loads(str(g['model_configs_json'])), scene_configs
