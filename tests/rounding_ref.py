"""CPU restatement of the 16-bit MLP kernels' ROUNDING -- test infrastructure, never imported by the package.

The fp32 oracle (oracle/nerf_oracle.py) is pinned to the reference project and answers "how far is a 16-bit mode from fp32".  This
module answers a different question: "is the kernel exactly the arithmetic it claims to be".  It evaluates an MLP in float64 and
rounds where OUR kernels round, to the format they round to, so that a kernel can be held to its own rounding noise instead of to
the much larger distance between its mode and fp32.

Every rounding goes float64 -> float32 -> 16-bit format: the kernels accumulate in fp32 and convert the fp32 result.  What is not
emulated, and why it does not matter:
  * the fp32 accumulation itself (the order of the kernels' sums): covered by the per-element bound ``sum_bound`` below;
  * the per-sample power-of-two renormalisation of the fused backward chain (mlp_backward_half_kernel.h, ``renormalise``):
    scaling by a power of two changes no rounding outside the subnormal range, so it is left out;
  * the fp16 range watch (mlp_device_f16.h, ``RangeWatch``): it only reports, it changes no value.

The mode table ``MODES`` lists, per kernel family, where it rounds and to what, each entry citing the source it restates (paths
relative to simplenerf_amd/csrc).
"""
from __future__ import annotations

import dataclasses
from typing import Dict, List, Optional

import torch

from oracle import nerf_oracle as oracle

F64 = torch.float64

# ----------------------------------------------------------------------------------------------------------- rounding helpers
# (mantissa bits, smallest normal exponent, largest finite value)
FORMATS = {
    'bf16': (7, -126, float.fromhex('0x1.fep127')),
    'fp16': (10, -14, 65504.0),
    'e4m3': (3, -6, 448.0),
    'fp32': (23, -126, float.fromhex('0x1.fffffep127')),
}
E4M3_CLAMP = 448.0        # store_pieces8 (mlp_device_f16.h:583-604): min(x, 448) before the fp8 conversion


def fp32(x: torch.Tensor) -> torch.Tensor:
    """float64 -> nearest float32 (ties to even), as float64."""
    return x.to(torch.float32).to(F64)


def _round(x: torch.Tensor, fmt: str) -> torch.Tensor:
    """Round to nearest, ties to even, with subnormals, from the float32 value of x.  Overflow gives +-inf."""
    man, emin, top = FORMATS[fmt]
    x = fp32(x.to(F64))
    a = x.abs()
    _, e = torch.frexp(a)                              # a = m 2^e, m in [0.5, 1): the leading bit is 2^(e-1)
    e = torch.clamp(e - 1, min=emin)                   # below the normal range the quantum stays that of 2^emin (subnormals)
    q = torch.ldexp(torch.ones_like(a), e - man)
    r = torch.round(a / q) * q                         # a / q is exact (power-of-two scaling); torch.round ties to even
    r = torch.where(r > top, torch.full_like(r, float('inf')), r)
    r = torch.where(torch.isfinite(a), r, a)
    return torch.copysign(r, x)


def bf16(x: torch.Tensor) -> torch.Tensor:
    return _round(x, 'bf16')


def fp16(x: torch.Tensor) -> torch.Tensor:
    return _round(x, 'fp16')


def e4m3(x: torch.Tensor) -> torch.Tensor:
    """fp8 e4m3 (OCP, 'fn': no infinities) with the kernels' clamp at 448 applied before the conversion."""
    x = fp32(x.to(F64))
    return _round(torch.clamp(x, min=-E4M3_CLAMP, max=E4M3_CLAMP), 'e4m3')


def f16x3_split(x: torch.Tensor):
    """The f16x3 operand split (mlp_forward_half_kernel.h:5-8): v = hi + lo, hi = fp16(v), lo = fp16(v - hi)."""
    x = fp32(x.to(F64))
    hi = fp16(x)
    return hi, fp16(fp32(x - hi))


ROUND = {'bf16': bf16, 'fp16': fp16, 'e4m3': e4m3, 'fp32': fp32, None: lambda x: x}


def ulp(v: torch.Tensor, fmt: str) -> torch.Tensor:
    """Spacing of `fmt` at |v| (the subnormal quantum below the normal range)."""
    man, emin, _ = FORMATS[fmt]
    _, e = torch.frexp(v.to(F64).abs())
    return torch.ldexp(torch.ones_like(v, dtype=F64), torch.clamp(e - 1, min=emin) - man)


def sum_bound(x: torch.Tensor, w: torch.Tensor, b: Optional[torch.Tensor], ref: torch.Tensor, fmt: str) -> torch.Tensor:
    """Per-element bound on |kernel - ref| for Y = round_fmt(act(X . W^T + b)) with exact float64 `ref` (the same rounding applied):
    an fp32 sum of K products plus the bias is within (K + 1) 2^-24 (sum_k |x_k w_k| + |b|) of the exact value (the standard
    recursive-summation bound, one rounding per addition; the bf16 / fp16 products themselves are exact in fp32), ReLU does not
    enlarge a difference, and the final rounding to `fmt` can add one spacing of `fmt` where the exact value sits near a midpoint."""
    k = x.shape[1]
    mag = x.abs() @ w.abs().t()
    if b is not None:
        mag = mag + b.abs()
    err = (k + 1) * 2.0 ** -24 * mag
    return err + ulp(ref.abs() + err, fmt)


# ----------------------------------------------------------------------------------------------------------------- mode table
@dataclasses.dataclass(frozen=True)
class Rounding:
    """Where one kernel family rounds, and to what (None: not rounded, i.e. fp32 in the kernel, exact here)."""
    fmt: Optional[str]              # the 16-bit operand format
    weights: bool                   # trunk, feature and views-layer weights as staged
    head_weights: bool              # pts_output / views_output weights
    encoding: bool                  # point and view encodings
    hidden: bool                    # hidden activations h_l, the feature vector and h_v as stored / fed on
    heads_from_rounded: bool        # heads read the rounded h_D / h_v (True) or the fp32 accumulator (False)
    dz: Optional[str]               # layer gradients dZ as the weight gradients (and bias sums) read them (bf16 in every 16-bit mode)
    dz_chain: Optional[str]         # dZ as the operand of the next input-gradient product (the backward chain)
    head_dz: Optional[str]          # the heads' fp32 dZ in the head weight gradients
    head_dz_chain: Optional[str]    # ... in the input-gradient product of d h_D / d h_v (None: fp32, with the fp32 head weights)
    head_bias_dz: Optional[str]     # ... in the head bias sums
    dfeature_stored: bool = False   # d h_D = round(round(dfeature . W_feat) + dout . W_out) (True) or one fp32 sum (False)
    x8: bool = False                # X operand of the trunk weight gradients h_1 .. h_D-1 in e4m3 (256-wide trunks)
    cites: tuple = ()


EXACT = Rounding(None, False, False, False, False, True, None, None, None, None, None)

MODES: Dict[str, Rounding] = {
    # layered path on bf16 operands, forward and backward
    'layered_bf16': Rounding(
        'bf16', weights=True, head_weights=True, encoding=True, hidden=True, heads_from_rounded=True, dz='bf16', dz_chain='bf16',
        head_dz='bf16', head_dz_chain='bf16', head_bias_dz=None, dfeature_stored=True,
        cites=('mlp_generic_bf16.hip:117-134 Stage16::store: every fp32 operand (weights, head weights, the heads\' dZ) is '
               'rounded to bf16 as staged (pack_bf16, v_cvt_pk_bf16_f32, :37-40)',
               'mlp_generic_kernels.h:12-14 store_as<bf16>: encodings (:66), h_l, the feature vector, h_v and every dZ stored as bf16',
               'mlp_generic_walk.h:77, :90 + mlp_generic_bf16.hip:8-10: the heads read the stored bf16 h_D / h_v and write fp32',
               'mlp_generic_bf16.hip:161-215 write_tile16: acc + bias (+ the bf16 value accumulated onto) in fp32, ReLU / gate, one rounding',
               'mlp_generic_walk.h:181, mlp_generic_bf16.hip:412: a head\'s bias sum reads its fp32 dZ, a layer\'s its bf16 dZ',
               'mlp_generic_walk.h:220, :227: d h_D = bf16(gate . (bf16(dfeature . W_feat) + dout . W_out)): two roundings')),
    # fused storing forward (training) and its backward chain + weight-gradient kernel
    'fused_f16': Rounding(
        'fp16', weights=True, head_weights=False, encoding=True, hidden=True, heads_from_rounded=False, dz='bf16', dz_chain='fp16',
        head_dz='bf16', head_dz_chain=None, head_bias_dz='bf16',
        cites=('mlp_forward_half_kernel.h:186-190, :217-220 convert_tile<.., BF>: h_l rounded to the 16-bit format (RNE, '
               'mlp_device_f16.h:30)',
               'mlp_forward_half_kernel.h:162-168, :282 heads_from / tile_dot_relu: the heads from the fp32 accumulator, fp32 head weights',
               'mlp_forward_half_kernel.h:244-256: feature from the rounded h_D, itself rounded (no ReLU)',
               'mlp_backward_half_kernel.h:110-135, :357 store_dy: the masked fp32 dY stored as bf16 for the weight gradients and bias '
               'sums (mlp_backward.hip:710-720 wgrad16_kernel: bf16 -> fp32 exact, bias sum, -> fp16 after a power-of-two region scale: '
               'exact); :225-228 the head dZ stored as bf16 likewise',
               'mlp_backward_half_kernel.h:266-270, :282-286, :324-336: the chain operand of the next product is the masked fp32 dY '
               'converted to the 16-bit format (convert_tile<false, BF>) after the per-sample power-of-two renormalisation',
               'mlp_backward_half_kernel.h:244-258, :300-322: d h_v and the density / colour rows of d h_D from the fp32 head dZ and '
               'fp32 head weights (VALU fma); d h_D = W_feat^T dfeature + W_out^T dsigma in one fp32 accumulator')),
    'fused_bf16': Rounding(
        'bf16', weights=True, head_weights=False, encoding=True, hidden=True, heads_from_rounded=False, dz='bf16', dz_chain='bf16',
        head_dz='bf16', head_dz_chain=None, head_bias_dz='bf16',
        cites=('as fused_f16, with BF = true: bf16 operands (mlp_forward_bf16.hip, mlp_backward_bf16.hip)',)),
    # the m16 inference kernel: the storing forward's rounding points, another fp32 accumulation order
    'm16_f16': Rounding(
        'fp16', weights=True, head_weights=False, encoding=True, hidden=True, heads_from_rounded=False, dz=None, dz_chain=None,
        head_dz=None, head_dz_chain=None, head_bias_dz=None,
        cites=('mlp_forward_m16_body.h:342, :373 tile_dot_relu16: heads from the fp32 accumulator',)),
    'm16_bf16': Rounding(
        'bf16', weights=True, head_weights=False, encoding=True, hidden=True, heads_from_rounded=False, dz=None, dz_chain=None,
        head_dz=None, head_dz_chain=None, head_bias_dz=None,
        cites=('as m16_f16 with bf16 operands',)),
}
MODES['fused_f16s8'] = dataclasses.replace(MODES['fused_f16'], x8=True, cites=(
    'mlp_forward_half_kernel.h:62-70, :188, :224 store_pieces8: h_1 .. h_D-1 of a 256-wide trunk saved as e4m3, min(x, 448) first '
    '(mlp_device_f16.h:569-604); only the weight gradients read them',))
MODES['fused_bf16s8'] = dataclasses.replace(MODES['fused_bf16'], x8=True, cites=MODES['fused_f16s8'].cites)


# ------------------------------------------------------------------------------------------------------------------- forward
def _linear(x, w, b):
    return x @ w.t() + (b if b is not None else 0.0)


def mlp_params64(sd: dict) -> Dict[str, torch.Tensor]:
    return {k: (v if isinstance(v, torch.Tensor) else torch.from_numpy(v)).to(F64) for k, v in sd.items()}


def encodings(cfg: dict, pts: torch.Tensor, view_dirs: Optional[torch.Tensor]):
    """float64 encodings of the float32 sample positions / view directions, (B, pe_full) and (B, views_pe) or None."""
    enc = oracle.pos_encode(pts.reshape(-1, 3).to(F64), cfg['points_positional_encoding_degree'])
    venc = None
    if view_dirs is not None and cfg.get('use_view_dirs', True) and cfg.get('view_dependent_rgb', True):
        venc = oracle.pos_encode(view_dirs.reshape(-1, 3).to(F64), cfg['views_positional_encoding_degree'])
    return enc, venc


def forward(params: Dict[str, torch.Tensor], cfg: dict, enc: torch.Tensor, venc: Optional[torch.Tensor],
            noise: Optional[torch.Tensor], mode: Rounding) -> dict:
    """The MLP of oracle.mlp_forward in float64 with `mode`'s rounding.  enc / venc: unrounded float64 encodings (``encodings``).
    -> {'sigma' (B,1), 'rgb' (B,3), 'layers': [{name, x, w, b, relu, pre, out}] in evaluation order}; `x` is the layer's input as
    fed (rounded), `w` the weight as staged, `pre` the exact pre-activation of those, `out` what the layer hands on."""
    r = ROUND[mode.fmt]
    rw = r if mode.weights else (lambda t: t)
    rh = r if mode.hidden else (lambda t: t)
    lay = oracle.mlp_layout(params, '')
    enc_r = r(enc) if mode.encoding else enc
    trunk_in = enc_r[:, :lay['pts_in']]
    layers = []

    def layer(name, x, relu, weights_rounded=True, out_rounded=True):
        w = params[f'{name}.weight']
        w = rw(w) if weights_rounded else w
        if not weights_rounded and mode.head_weights:
            w = r(w)
        b = params[f'{name}.bias']
        pre = _linear(x, w, b)
        act = torch.relu(pre) if relu else pre
        out = rh(act) if out_rounded else act
        layers.append({'name': name, 'x': x, 'w': w, 'b': b, 'relu': relu, 'pre': pre, 'out': out})
        return act, out

    h = trunk_in
    act = None
    for i in range(lay['depth']):
        act, h = layer(f'pts_linears.{i}', h, True)
        if i == oracle.SKIP_AFTER_LAYER and lay['depth'] > oracle.SKIP_AFTER_LAYER + 1:
            h = torch.cat([trunk_in, h], -1)
    h_head = h if mode.heads_from_rounded else act
    head, _ = layer('pts_output_linear', h_head, False, weights_rounded=False, out_rounded=False)
    sigma = head[:, 0:1] + (noise.reshape(-1, 1).to(F64) if noise is not None else 0.0)
    out = {'sigma': torch.relu(sigma), 'layers': layers, 'head': head}
    if lay['pts_out'] == 4:
        out['rgb'] = torch.sigmoid(head[:, 1:4])
    if lay['view_dependent']:
        _, feature = layer('feature_linear', h, False)
        hv = torch.cat([feature, enc_r[:, lay['pts_in']:], r(venc) if mode.encoding else venc], -1)
        act_v = None
        for j in range(lay['views_depth']):
            act_v, hv = layer(f'views_linears.{j}', hv, True)
        vhead, _ = layer('views_output_linear', hv if mode.heads_from_rounded else act_v, False, weights_rounded=False,
                         out_rounded=False)
        out['vhead'] = vhead
        out['rgb'] = torch.sigmoid(vhead[:, 0:3])
    return out


# ------------------------------------------------------------------------------------------------------------------ backward
def heads_backward(sigma: torch.Tensor, rgb: torch.Tensor, d_sigma: torch.Tensor, d_rgb: torch.Tensor, view_dep: bool, exact: bool):
    """dL/d(head outputs) from sigma (B,1), rgb (B,3) and the upstream gradients, as mlp_generic_kernels.h:86-104 (fp32 steps,
    each rounded to fp32 unless `exact`).  -> dout (B, 4 or 1), dvout (B, 3) or None"""
    f = (lambda t: t) if exact else fp32
    s, c = sigma.reshape(-1, 1).to(F64), rgb.reshape(-1, 3).to(F64)
    col = f(d_rgb.reshape(-1, 3).to(F64) * f(c * f(1.0 - c)))
    dsig = d_sigma.reshape(-1, 1).to(F64) * (s > 0)
    if view_dep:
        return dsig, col
    return torch.cat([dsig, col], 1), None


def backward(params: Dict[str, torch.Tensor], cfg: dict, layers: List[dict], dout: torch.Tensor, dvout: Optional[torch.Tensor],
             mode: Rounding, operands: Optional[dict] = None) -> Dict[str, torch.Tensor]:
    """Every parameter gradient, in float64 with `mode`'s rounding of dZ (as the weight gradients read it, and as the chain's next
    product reads it) and of the X operand of the weight gradients.  `layers`: the forward's records (``forward``), or the same built
    from a kernel's saved tensors -- `x` is the weight gradient's X, `out` the layer's stored output, `mask` (optional; default
    out > 0) its ReLU gate, `w` the weight as staged.  dout: (B, pts_out) (the density row, and the colour rows of a
    view-independent MLP), dvout: (B, 3) or None.  `operands`: if a dict, receives each weight gradient's (dZ, X, bias dZ) as
    multiplied, by layer name (for summation bounds)."""
    lay = oracle.mlp_layout(params, '')
    by = {L['name']: L for L in layers}
    rz, rc = ROUND[mode.dz], ROUND[mode.dz_chain]
    rhd, rhc, rhb = ROUND[mode.head_dz], ROUND[mode.head_dz_chain], ROUND[mode.head_bias_dz]
    width = lay['width']
    grads = {}

    def gate(L):
        return L['mask'] if 'mask' in L else L['out'] > 0

    def wgrad(name, dz, dz_for_bias, x):
        grads[f'{name}.weight'] = dz.t() @ x
        if operands is not None:
            operands[name] = (dz, x, dz_for_bias)
        grads[f'{name}.bias'] = dz_for_bias.sum(0)

    def x8(name, x):
        """the s8 modes' X operand: h_1 .. h_D-1 of a 256-wide trunk (the input of trunk layers 1 .. D-1, skip block included)"""
        if not (mode.x8 and name.startswith('pts_linears.') and width == 256 and name != 'pts_linears.0'):
            return x
        if name == f'pts_linears.{oracle.SKIP_AFTER_LAYER + 1}' and lay['depth'] > oracle.SKIP_AFTER_LAYER + 1:
            return torch.cat([x[:, :lay['pts_in']], e4m3(x[:, lay['pts_in']:])], 1)
        return e4m3(x)

    last = by[f'pts_linears.{lay["depth"] - 1}']
    h_last = last['out']                                  # h_D as saved (the fused heads read the fp32 accumulator)
    dh_extra = 0.0
    if lay['view_dependent']:
        vo = by['views_output_linear']
        hv_last = by[f'views_linears.{lay["views_depth"] - 1}']
        wgrad('views_output_linear', rhd(dvout), rhb(dvout), hv_last['out'])
        dy = (rhc(dvout) @ vo['w']) * gate(hv_last)      # the masked fp32 dY of the last views layer
        for j in range(lay['views_depth'] - 1, -1, -1):
            L = by[f'views_linears.{j}']
            wgrad(L['name'], rz(dy), rz(dy), L['x'])
            if j > 0:
                dy = (rc(dy) @ L['w']) * gate(by[f'views_linears.{j - 1}'])
            else:
                dy = rc(dy) @ L['w'][:, :width]
        F_ = by['feature_linear']
        wgrad('feature_linear', rz(dy), rz(dy), F_['x'])
        dh_extra = rc(dy) @ F_['w']
        if mode.dfeature_stored:
            dh_extra = rz(dh_extra)
    po = by['pts_output_linear']
    wgrad('pts_output_linear', rhd(dout), rhb(dout), h_last)
    dy = (rhc(dout) @ po['w'] + dh_extra) * gate(last)
    for l in range(lay['depth'] - 1, -1, -1):
        L = by[f'pts_linears.{l}']
        wgrad(L['name'], rz(dy), rz(dy), x8(L['name'], L['x']))
        if l == 0:
            break
        dy = (rc(dy) @ L['w'][:, -width:]) * gate(by[f'pts_linears.{l - 1}'])   # the skip layer's input is [encoding | H_l-1]
    return grads
