"""The 16-bit MLP kernels against a float64 reference that rounds where they round (tests/rounding_ref.py) -- a tolerance class of its
own, "against the kernel's own rounding" (DESIGN §4).  The fp32-relative tests (test_gpu_bf16.py, test_gpu_f16.py,
test_gpu_layered_bf16.py) stay: they measure how far each mode is from fp32, which is a different question, and their gates are as
wide as that distance.  The gates here are set by the modes' own rounding noise, so that a kernel wrong by less than the distance
to fp32 -- a dropped k-group, a wrongly padded tail tile, truncation instead of round-to-nearest-even, a misplaced fp8 clamp, a bias
sum missing a row chunk -- fails them.

  a. layer by layer from the kernel's own saved tensors (layered bf16; fused f16 / bf16): each layer's output recomputed in float64 from the saved
     input of that layer and the rounded weights: every element within rounding_ref.sum_bound, and most bit-equal;
  b. sigma / rgb of every 16-bit family against the emulated forward;
  c. parameter gradients against the emulated backward, with the kernel's own saved activations and ReLU masks (layered bf16, and
     the fused f16 / bf16 pieces and mask words);
     backward(into=...) against prior + fresh; the s8 modes' clamped e4m3 operand through g_s8 - g_16;
  d. the layered GEMMs across their tile and split-K thresholds, fp32 and bf16: a whole call against the sum over its parts, the
     instance each call takes computed here from the kernels' own formulas and asserted;
  e. seeded ragged sweeps of the 16-bit modes.

Gates: each at most its ceiling (an error estimate: a rounding disagreement at a bf16 midpoint moves a layer output by about 1e-4
of its scale) and at most 4x the worst value observed on the MI355X.  Observed figures are printed in pytest's summary (tag
`rounding/...`).  Measured on the MI355X:
  a. every layer within its bound (worst 1.00 of it: a one-ulp midpoint disagreement), >= 99.99 % of each layer bit-equal;
  b. sigma / rgb: bf16 4.1e-4 of max / 3.0e-5 (layered, fused, m16), f16 1.4e-4 / 2.6e-6 (fused, f16s8, m16);
     fused sigma / rgb from the kernel's own saved head inputs 5.0e-7 of max / 6.6e-8;
  c. gradients with the kernel's own masks (layered bf16; fused f16 / bf16: the backward chain and wgrad16_kernel) 2.3e-3 of max,
     9.5e-4 rel L2; into= 1.0 fp32 ulp (4.5 before the split reduction added the prior last, csrc/mlp_generic_kernels.h
     reduce_splits_kernel); s8 clamp g_s8 - g_16 7.6e-4 rel L2;
  d. whole call vs parts 4.1e-6 of max, every element within its summation bound.
The s8 modes' e4m3 saved trunk is not decoded: their forward is held bit-equal to the 16-bit mode's and the clamp through
g_s8 - g_16."""
import numpy
import pytest
import torch

from oracle import nerf_oracle as oracle
from simplenerf_amd import ops, synth
from tests import rounding_ref as rr
from tests import util
from tests.test_gpu_generic import SHAPES, case
from tests.test_gpu_grads import rel_l2, rel_to_max
from tests.test_gpu_kernels import LAYOUTS

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
P = ops.PRECISIONS

# gates (ceiling of the issue in brackets where it differs): see the module docstring
BIT_EQUAL_MIN = 0.99                 # fraction of the elements of a layer bit-equal to the float64 reference (observed >= 0.9999)
OUT_GATES = {'bf16': (1.6e-3, 5e-5), 'fp16': (5e-4, 1e-5)}   # sigma rel-to-max, rgb max abs [2e-3, 5e-5; 5e-4, 1e-5]
GRAD_REL_MAX, GRAD_REL_L2 = 4.8e-3, 2e-3                     # identical masks [5e-3, 2e-3]
INTO_ULPS = 2.0                                              # into=: fp32 ulps of max(|prior|, |fresh|)
WHOLE_VS_PARTS = 1.6e-5                                      # of a gradient tensor's largest entry [1e-4]
S8_DELTA_L2 = 3e-3                                           # the s8 operand's effect on a weight gradient [2e-2]
HEADS_GATES = (2e-6, 2.6e-7)                                 # fused sigma / rgb from the kernel's saved head inputs


# ------------------------------------------------------------------------------------------------- the layered path's saved row
def plan_of(cfg):
    """GenericPlan's sizes (csrc/mlp_generic.hip:60-92)"""
    view_dep = bool(cfg['view_dependent_rgb'])
    p = {'depth': cfg['points_net_depth'], 'width': cfg['points_net_width'], 'view_dep': view_dep,
         'views_depth': cfg['views_net_depth'] if view_dep else 0, 'views_width': cfg['views_net_width'] if view_dep else 0}
    p['pe_full'] = 3 + 6 * cfg['points_positional_encoding_degree']
    p['pts_in'] = (2 * cfg['points_sigma_positional_encoding_degree'] + 1) * 3 if 'points_sigma_positional_encoding_degree' in cfg \
        else p['pe_full']
    p['extra'] = p['pe_full'] - p['pts_in']
    p['views_pe'] = 3 + 6 * cfg['views_positional_encoding_degree'] if p['view_dep'] else 0
    p['views_in'] = p['width'] + p['extra'] + p['views_pe']
    return p


def generic_row(p, align, heads_in_row):
    """generic_row (csrc/mlp_generic.hip:700-719): column of every block of one sample's activation row"""
    c = 0
    r = {'c_h': [], 'c_hv': []}

    def nxt(c):
        return (c + align - 1) // align * align
    r['c_pe'] = c; c += p['pe_full']
    c = nxt(c); r['c_pev'] = c; c += p['views_pe']
    r['c_x5'] = -1
    for l in range(p['depth']):
        c = nxt(c)
        if l == 4 and p['depth'] > 5:
            r['c_x5'] = c; c += p['pts_in']
        r['c_h'].append(c); c += p['width']
    c = nxt(c); r['c_v0'] = c
    if p['view_dep']:
        c += p['views_in']
    for _ in range(p['views_depth']):
        c = nxt(c); r['c_hv'].append(c); c += p['views_width']
    c = nxt(c)
    if heads_in_row:
        r['c_out'] = c; c += 8
    r['row'] = c
    return r


def decode_layered(saved, cfg, total, bf16):
    """The layered path's saved tensor -> {'row': (total, row) float64 activation matrix, 'heads': (total, 8) fp32 head outputs,
    'r': the column map}.  bf16: a bf16 matrix, rows of multiples of eight, then an fp32 [N][8] heads block after its whole 16-byte
    groups (csrc/mlp_generic_bf16.hip:8-11, mlp_generic_walk.h:53-57); fp32: the heads in the row (kHeadsInRow)."""
    p = plan_of(cfg)
    r = generic_row(p, 8 if bf16 else 4, not bf16)
    if bf16:
        elems = total * r['row']
        matrix_floats = (elems + 7) // 8 * 4
        bits = saved[:matrix_floats].view(torch.int16)[:elems].reshape(total, r['row']).cpu()
        row = (bits.to(torch.int32) << 16).view(torch.float32).double()
        heads = saved[matrix_floats:matrix_floats + 8 * total].reshape(total, 8).cpu().double()
    else:
        row = saved[:total * r['row']].reshape(total, r['row']).cpu().double()
        heads = row[:, r['c_out']:r['c_out'] + 8]
    return {'row': row, 'heads': heads, 'r': r, 'p': p}


def layered_records(sd, cfg, dec, mode):
    """rounding_ref layer records built from the kernel's saved tensors: each layer's input x and output `out` as the kernel stored
    them, w as staged, pre = x . w^T + b exact."""
    p, r, row = dec['p'], dec['r'], dec['row']
    params = rr.mlp_params64(sd)
    rw = rr.ROUND[mode.fmt] if mode.weights else (lambda t: t)
    rhw = rr.ROUND[mode.fmt] if mode.head_weights else (lambda t: t)
    cols = lambda c, n: row[:, c:c + n]
    recs = []

    def rec(name, x, out, relu, head=False):
        w = (rhw if head else rw)(params[f'{name}.weight'])
        b = params[f'{name}.bias']
        recs.append({'name': name, 'x': x, 'w': w, 'b': b, 'relu': relu, 'pre': x @ w.t() + b, 'out': out, 'head': head})

    for l in range(p['depth']):
        if l == 0:
            x = cols(r['c_pe'], p['pts_in'])
        elif l == 5 and p['depth'] > 5:
            x = cols(r['c_x5'], p['pts_in'] + p['width'])
        else:
            x = cols(r['c_h'][l - 1], p['width'])
        rec(f'pts_linears.{l}', x, cols(r['c_h'][l], p['width']), True)
    h_last = cols(r['c_h'][-1], p['width'])
    rows = 1 if p['view_dep'] else 4
    rec('pts_output_linear', h_last, dec['heads'][:, 0:rows], False, head=True)
    if p['view_dep']:
        rec('feature_linear', h_last, cols(r['c_v0'], p['width']), False)
        for j in range(p['views_depth']):
            x = cols(r['c_v0'], p['views_in']) if j == 0 else cols(r['c_hv'][j - 1], p['views_width'])
            rec(f'views_linears.{j}', x, cols(r['c_hv'][j], p['views_width']), True)
        rec('views_output_linear', cols(r['c_hv'][-1], p['views_width']), dec['heads'][:, 4:7], False, head=True)
    return recs


def check_layers(recs, fmt, tag):
    """2a: every element within the bound, at least BIT_EQUAL_MIN of each 16-bit layer bit-equal.  -> (worst bound use, worst
    bit-equal fraction)"""
    worst_use, worst_eq = 0.0, 1.0
    for L in recs:
        if L['out'] is None:
            continue
        f = 'fp32' if L['head'] else fmt
        act = torch.relu(L['pre']) if L['relu'] else L['pre']
        ref = rr.ROUND[f](act)
        got = L['out']
        bound = rr.sum_bound(L['x'], L['w'], L['b'], ref, f)
        use = float(((got - ref).abs() / bound).max())
        worst_use = max(worst_use, use)
        assert use <= 1.0, (tag, L['name'], use, int(((got - ref).abs() > bound).sum()))
        if not L['head'] and fmt != 'fp32':
            eq = float((got == ref).double().mean())
            worst_eq = min(worst_eq, eq)
            assert eq >= BIT_EQUAL_MIN, (tag, L['name'], eq)
    return worst_use, worst_eq


def packed(cfg, sd):
    plist = synth.abi_param_list({k: torch.from_numpy(a).to(DEV) for k, a in sd.items()})
    mlp = ops.PackedMlp(cfg, DEV)
    mlp.pack(plist)
    return mlp, [tuple(t.shape) for t in plist]


def emulated(cfg, sd, inputs, mode):
    o, d, v, z, noise = inputs
    pts = oracle.ray_points(o, d, z)
    vd = v[:, None].expand(pts.shape) if cfg['use_view_dirs'] else None
    enc, venc = rr.encodings(cfg, pts, vd)
    return rr.forward(rr.mlp_params64(sd), cfg, enc, venc, noise, mode)


def compare_outputs(sigma, rgb, ref, fmt, tag, gates=None):
    s_gate, c_gate = gates or OUT_GATES[fmt]
    e_s = rel_to_max(sigma.reshape(-1, 1), ref['sigma'])
    e_c = util.linf(rgb.reshape(-1, 3).cpu().double(), ref['rgb'])
    util.observe(f'rounding/{tag}', f'sigma {e_s:.1e} of max [{s_gate}], rgb {e_c:.1e} [{c_gate}]')
    assert e_s <= s_gate and e_c <= c_gate, (tag, e_s, e_c)
    return e_s, e_c


def compare_grads(got, want, names, tag, rel_max=GRAD_REL_MAX, rel2=GRAD_REL_L2):
    worst_m, worst_2 = 0.0, 0.0
    for name, g in zip(names, got):
        w = want[name]
        if float(w.abs().max()) == 0:
            assert float(g.abs().max()) == 0, (tag, name)
            continue
        m, l2 = rel_to_max(g, w), rel_l2(g, w)
        worst_m, worst_2 = max(worst_m, m), max(worst_2, l2)
        assert m <= rel_max and l2 <= rel2, (tag, name, m, l2)
    util.observe(f'rounding/{tag}', f'gradients {worst_m:.1e} of max [{rel_max}], rel L2 {worst_2:.1e} [{rel2}]')


def layered_case_checks(cfg, sd, inputs, grads_in, tag, layers=True, outputs=True, gradients=True):
    """2a + 2b + 2c of one layered bf16 case."""
    mode = rr.MODES['layered_bf16']
    mlp, shapes = packed(cfg, sd)
    dev = [t.to(DEV) for t in inputs]
    n, s = inputs[3].shape
    sigma, rgb, saved = mlp.forward_train(*dev, P['bf16'])
    dec = decode_layered(saved, cfg, n * s, True)
    recs = layered_records(sd, cfg, dec, mode)
    if layers:
        use, eq = check_layers(recs, 'bf16', tag)
        util.observe(f'rounding/{tag}/layers', f'worst |err| / bound {use:.2f} [1], worst bit-equal fraction {eq:.4f} [{BIT_EQUAL_MIN}]')
    if outputs:
        compare_outputs(sigma, rgb, emulated(cfg, sd, inputs, mode), 'bf16', f'{tag}/outputs')
    if gradients:
        g_sigma, g_rgb = grads_in
        got = mlp.backward(saved, sigma, rgb, g_sigma.to(DEV), g_rgb.to(DEV), shapes, P['bf16'])
        want = reference_grads(sd, cfg, recs, sigma, rgb, g_sigma, g_rgb, mode)
        compare_grads(got, want, synth.abi_param_list({k: k for k in sd}), f'{tag}/gradients')
    return mlp, shapes, dev, (sigma, rgb, saved), recs


def reference_grads(sd, cfg, recs, sigma, rgb, g_sigma, g_rgb, mode, operands=None):
    dout, dvout = rr.heads_backward(sigma.cpu(), rgb.cpu(), g_sigma, g_rgb, bool(cfg['view_dependent_rgb']), exact=False)
    return rr.backward(rr.mlp_params64(sd), cfg, recs, dout, dvout, mode, operands)


# ------------------------------------------------------------------------------------------------ a-c: the layered bf16 path
@pytest.mark.parametrize('index', range(len(SHAPES)))
def test_layered_bf16_against_its_own_rounding(index):
    cfg, sd, inputs, grads_in = case(index, 5, 37)
    layered_case_checks(cfg, sd, inputs, grads_in, f'layered_bf16/{index}/5x37')


def test_layered_bf16_accumulating_backward_adds_to_prior():
    """backward(into=...): each element equals prior + fresh within 2 fp32 ulps of max(|prior|, |fresh|)."""
    cfg, sd, inputs, (g_sigma, g_rgb) = case(2, 5, 37)
    accumulate_check(cfg, sd, inputs, g_sigma, g_rgb, P['bf16'], 'layered_bf16/2')


def accumulate_check(cfg, sd, inputs, g_sigma, g_rgb, prec, tag):
    mlp, shapes = packed(cfg, sd)
    dev = [t.to(DEV) for t in inputs]
    sigma, rgb, saved = mlp.forward_train(*dev, prec)
    fresh = mlp.backward(saved, sigma, rgb, g_sigma.to(DEV), g_rgb.to(DEV), shapes, prec)
    gen = torch.Generator(device=DEV).manual_seed(3)
    prior = [torch.randn(s, device=DEV, generator=gen) * float(f.abs().max()) for s, f in zip(shapes, fresh)]
    into = [t.clone() for t in prior]
    mlp.backward(saved, sigma, rgb, g_sigma.to(DEV), g_rgb.to(DEV), shapes, prec, into=into)
    worst = 0.0
    for a, p_, f in zip(into, prior, fresh):
        want = p_.double() + f.double()
        scale = torch.maximum(p_.abs(), f.abs()).double()
        ulps = ((a.double() - want).abs() / (scale * 2.0 ** -23).clamp_min(2.0 ** -149))
        worst = max(worst, float(ulps.max()))
    util.observe(f'rounding/{tag}/into', f'accumulated - (prior + fresh): {worst:.2f} fp32 ulps of max(|prior|, |fresh|) [{INTO_ULPS}]')
    assert worst <= INTO_ULPS


# ------------------------------------------------------------------------------------------------ b, c: the fused kernels
FUSED = [('main', (8, 256, 128)), ('main', (4, 128, 64))]
FUSED_MODES = {'f16': 'fused_f16', 'bf16': 'fused_bf16', 'f16s8': 'fused_f16s8', 'bf16s8': 'fused_bf16s8'}


def fused_case(layout, size, n=7, s=45, seed=31):
    depth, width, vwidth = size
    cfg = synth.mlp_config(64, depth=depth, width=width, views_width=vwidth, **LAYOUTS[layout])
    sd = synth.synth_state_dict(util.mlp_param_shapes(cfg), seed, 50.0, 1.0)
    rng = numpy.random.RandomState(depth + seed)
    o = torch.from_numpy(rng.uniform(-1, 1, (n, 3)).astype(numpy.float32))
    d = torch.from_numpy(rng.uniform(-1, 1, (n, 3)).astype(numpy.float32))
    v = d / d.norm(dim=1, keepdim=True)
    z = torch.from_numpy(numpy.sort(rng.uniform(0, 1, (n, s)).astype(numpy.float32), axis=1))
    noise = torch.from_numpy(rng.standard_normal((n, s, 1)).astype(numpy.float32))
    g_sigma = torch.from_numpy(rng.standard_normal((n, s, 1)).astype(numpy.float32))
    g_rgb = torch.from_numpy(rng.standard_normal((n, s, 3)).astype(numpy.float32))
    return cfg, sd, (o, d, v, z, noise), (g_sigma, g_rgb)


@pytest.mark.parametrize('precision', list(FUSED_MODES))
@pytest.mark.parametrize('layout,size', FUSED)
def test_fused_storing_forward_against_its_own_rounding(layout, size, precision):
    """2b: the storing (training) forward's sigma / rgb against the emulated forward of the mode."""
    cfg, sd, inputs, _ = fused_case(layout, size)
    mode = rr.MODES[FUSED_MODES[precision]]
    mlp, _ = packed(cfg, sd)
    sigma, rgb, _ = mlp.forward_train(*[t.to(DEV) for t in inputs], P[precision])
    compare_outputs(sigma, rgb, emulated(cfg, sd, inputs, mode), mode.fmt, f'fused/{layout}/{size[0]}x{size[1]}/{precision}')


# ---- the fused storing forward's saved tensor: 16-bit pieces and ReLU mask words (csrc/mlp_plan.h:61-79, mlp_device_f16.h:546-550)
def pe_feature(n, h, pairs, degree):
    """snerf::pe_feature (csrc/mlp_layout.h:36-50): reference encoding index of PE register n in lane half h, -1 for padding"""
    if n < pairs:
        c = (n >> 1) * 2 + h
        if c >= pairs or c // 3 >= degree:
            return -1
        return 3 + 6 * (c // 3) + 3 * (n & 1) + c % 3
    return {0: 0, 1: 2, 2: 1}.get((n - pairs) * 2 + h, -1)


def decode_fused(saved, cfg, total, bf16, blocks=None):
    """forward_train's saved tensor of the fused 16-bit modes -> natural-order float64 activations and bool masks per sample.
    Per 32-sample wave block, act16_rows rows of 32 x 16 bit: pe (4 pieces) | pev (2) | h_1 .. h_D | feature | h_v | mask words.
    A 1-KiB piece is one 16-feature k-step, [slot = 2 sample + lane half][8 elements]: element e of half h is feature
    16 p + 8 (e >> 2) + 4 h + (e & 3) of an activation, PE register 8 p + e of an encoding.  Mask word pair t >> 1, lane
    sample + 32 half, bit 16 (t & 1) + r <-> feature 32 u + (r & 3) + 8 (r >> 2) + 4 half of tile t (test_gpu_grads.py:136-154).
    `blocks`: wave-block indices to decode (gathered on the device, so only they move to the host); the rows are then the real
    samples of those blocks in order, their indices in dec['samples']."""
    p = plan_of(cfg)
    D, W, vw = p['depth'], p['width'], p['views_width']
    act_mask = 96 + (D + 1) * W + vw
    tiles = D * (W // 32) + vw // 32
    rows = act_mask + 4 * ((tiles + 1) // 2)
    halfs = saved.view(torch.int16)                  # (sized for the fp32 layout's longer blocks: the 16-bit blocks use its front)
    all_blocks = -(-total // 32)
    assert all_blocks * rows * 32 <= halfs.numel(), (halfs.numel(), rows, total)
    blk = halfs[:all_blocks * rows * 32].reshape(all_blocks, rows * 32)
    index = torch.arange(all_blocks) if blocks is None else torch.as_tensor(list(blocks), dtype=torch.int64)
    assert index.numel() == 0 or (0 <= int(index.min()) and int(index.max()) < all_blocks), (blocks, all_blocks)
    blk = (blk if blocks is None else blk[index.to(blk.device)]).cpu()
    blocks = index.numel()
    samples = (index[:, None] * 32 + torch.arange(32)).reshape(-1)
    live = samples < total                           # (all but the tail of the call's last block)
    samples, total = samples[live], int(live.sum())

    def value(bits):
        if bf16:
            return (bits.to(torch.int32) << 16).view(torch.float32).double()
        return bits.view(torch.float16).double()

    def region(r0, nfeat):
        x = blk[:, r0 * 32:(r0 + nfeat) * 32].reshape(blocks, nfeat // 16, 32, 2, 2, 4)      # piece, sample, h, g, q
        return value(x.permute(0, 2, 1, 4, 3, 5).reshape(blocks * 32, nfeat)[live].contiguous())

    def encoding(r0, npieces, pairs, degree, nfeat):
        raw = value(blk[:, r0 * 32:r0 * 32 + npieces * 512].reshape(blocks, npieces, 32, 2, 8).permute(0, 2, 1, 3, 4)
                    .reshape(blocks * 32, npieces * 16)[live].contiguous())              # column 16 p + 8 h + e
        out = torch.zeros(total, nfeat, dtype=torch.float64)
        for q in range(npieces):
            for h in range(2):
                for e in range(8):
                    f = pe_feature(8 * q + e, h, pairs, degree)
                    if f >= 0:
                        out[:, f] = raw[:, 16 * q + 8 * h + e]
        return out

    words = blk[:, act_mask * 32:act_mask * 32 + ((tiles + 1) // 2) * 128].contiguous().view(torch.int32).to(torch.int64) & 0xffffffff
    words = words.reshape(blocks, (tiles + 1) // 2, 2, 32)                                   # pair, half, sample

    def masks(t0, ntiles):
        out = torch.zeros(blocks, 32, ntiles * 32, dtype=torch.bool)
        for u in range(ntiles):
            t = t0 + u
            for h in range(2):
                for r in range(16):
                    out[:, :, 32 * u + (r & 3) + 8 * (r >> 2) + 4 * h] = ((words[:, t >> 1, h, :] >> (16 * (t & 1) + r)) & 1).bool()
        return out.reshape(blocks * 32, ntiles * 32)[live]

    pe_full = p['pe_full']
    dec = {'samples': samples, 'pe': encoding(0, 4, 30, cfg['points_positional_encoding_degree'], pe_full),
           'h': [region(96 + l * W, W) for l in range(D)], 'mask': [masks(l * (W // 32), W // 32) for l in range(D)]}
    if p['view_dep']:
        dec['pev'] = encoding(64, 2, 12, cfg['views_positional_encoding_degree'], p['views_pe'])
        dec['feature'] = region(96 + D * W, W)
        dec['hv'] = region(96 + (D + 1) * W, vw)
        dec['vmask'] = masks(D * (W // 32), vw // 32)
    return dec


def fused_records(sd, cfg, dec, mode):
    """rounding_ref layer records from the fused kernels' saved tensors (as layered_records); the heads read the fp32 accumulator,
    which is not saved: their records carry the saved h_D / h_v as the weight gradients' X and no output to check."""
    p = plan_of(cfg)
    params = rr.mlp_params64(sd)
    r = rr.ROUND[mode.fmt]
    recs = []

    def rec(name, x, out, relu, mask=None, head=False):
        w = params[f'{name}.weight']
        w = r(w) if (mode.head_weights if head else mode.weights) else w
        b = params[f'{name}.bias']
        L = {'name': name, 'x': x, 'w': w, 'b': b, 'relu': relu, 'pre': x @ w.t() + b, 'out': out, 'head': head}
        if mask is not None:
            L['mask'] = mask
        recs.append(L)

    pe, h = dec['pe'], dec['h']
    for l in range(p['depth']):
        if l == 0:
            x = pe[:, :p['pts_in']]
        elif l == 5 and p['depth'] > 5:
            x = torch.cat([pe[:, :p['pts_in']], h[4]], 1)
        else:
            x = h[l - 1]
        rec(f'pts_linears.{l}', x, h[l], True, dec['mask'][l])
    rec('pts_output_linear', h[-1], None, False, head=True)
    if p['view_dep']:
        rec('feature_linear', h[-1], dec['feature'], False)
        rec('views_linears.0', torch.cat([dec['feature'], pe[:, p['pts_in']:], dec['pev']], 1), dec['hv'], True, dec['vmask'])
        rec('views_output_linear', dec['hv'], None, False, head=True)
    return recs


def heads_from_saved(recs, cfg, noise):
    """sigma / rgb of the fused heads recomputed from the kernel's own saved inputs of the last trunk and views layers: ReLU of the
    exact pre-activation (the heads read the fp32 accumulator) times the fp32 head weights."""
    p = plan_of(cfg)
    by = {L['name']: L for L in recs}
    po = by['pts_output_linear']
    head = torch.relu(by[f'pts_linears.{p["depth"] - 1}']['pre']) @ po['w'].t() + po['b']
    out = {'sigma': torch.relu(head[:, 0:1] + noise.reshape(-1, 1).double())}
    if p['view_dep']:
        vo = by['views_output_linear']
        out['rgb'] = torch.sigmoid(torch.relu(by['views_linears.0']['pre']) @ vo['w'].t() + vo['b'])[:, :3]
    else:
        out['rgb'] = torch.sigmoid(head[:, 1:4])
    return out


def fused_layers_and_gradients(cfg, sd, inputs, grads_in, precision, tag, gradients=True):
    """2a and 2c of one fused case in 'f16' or 'bf16' (the s8 modes keep h_1 .. h_D-1 as e4m3, which this decoder does not read)."""
    mode = rr.MODES[FUSED_MODES[precision]]
    mlp, shapes = packed(cfg, sd)
    dev = [t.to(DEV) for t in inputs]
    n, s = inputs[3].shape
    sigma, rgb, saved = mlp.forward_train(*dev, P[precision])
    recs = fused_records(sd, cfg, decode_fused(saved, cfg, n * s, mode.fmt == 'bf16'), mode)
    for L in recs:                                   # the mask words are the signs of what was stored, up to an underflow to zero
        if 'mask' in L:
            assert not bool((L['out'] > 0)[~L['mask']].any()), (tag, L['name'])
    use, eq = check_layers(recs, mode.fmt, tag)
    util.observe(f'rounding/{tag}/layers', f'worst |err| / bound {use:.2f} [1], worst bit-equal fraction {eq:.4f} [{BIT_EQUAL_MIN}]')
    compare_outputs(sigma, rgb, heads_from_saved(recs, cfg, inputs[4]), mode.fmt, f'{tag}/heads', HEADS_GATES)
    if gradients:
        g_sigma, g_rgb = grads_in
        got = mlp.backward(saved, sigma, rgb, g_sigma.to(DEV), g_rgb.to(DEV), shapes, P[precision])
        want = reference_grads(sd, cfg, recs, sigma, rgb, g_sigma, g_rgb, mode)
        compare_grads(got, want, synth.abi_param_list({k: k for k in sd}), f'{tag}/gradients')
    return recs


@pytest.mark.parametrize('n,s', [(5, 37), (64, 129)])
@pytest.mark.parametrize('precision', ['f16', 'bf16'])
@pytest.mark.parametrize('layout,size', FUSED)
def test_fused_layers_and_gradients_against_their_own_rounding(layout, size, precision, n, s):
    """2a on the fused storing forward (every layer from the kernel's own saved input) and 2c on its backward chain and the
    weight-gradient kernel (wgrad16_kernel), with the kernel's own saved activations and ReLU mask words."""
    cfg, sd, inputs, grads_in = fused_case(layout, size, n, s)
    fused_layers_and_gradients(cfg, sd, inputs, grads_in, precision, f'fused/{layout}/{size[0]}x{size[1]}/{precision}/{n}x{s}')


@pytest.mark.parametrize('precision', ['f16', 'bf16'])
def test_m16_inference_kernel_against_its_own_rounding(precision):
    """2b for the 16x16x32-MFMA inference kernel of the main 8x256 layout (PackedMlp.forward)."""
    cfg, sd, inputs, _ = fused_case('main', (8, 256, 128))
    mlp, _ = packed(cfg, sd)
    sigma, rgb = mlp.forward(*[t.to(DEV) for t in inputs], P[precision])
    mode = rr.MODES[f'm16_{precision}']
    compare_outputs(sigma, rgb, emulated(cfg, sd, inputs, mode), mode.fmt, f'm16/{precision}')


def test_fused_accumulating_backward_adds_to_prior():
    cfg, sd, inputs, (g_sigma, g_rgb) = fused_case('main', (8, 256, 128))
    accumulate_check(cfg, sd, inputs, g_sigma, g_rgb, P['bf16'], 'fused/main/8x256/bf16')


# ------------------------------------------------------------------------------- d: the layered GEMMs across their thresholds
def gemm_tile(M, N, splits):
    """gemm_grid (csrc/mlp_generic_walk.h:31-35)"""
    large = -(-N // 128) * -(-M // 128) * max(splits, 1)
    return 128 if M >= 128 and N >= 128 and large >= 512 else 64


def wgrad_splits(total):
    """generic_wgrad_splits (csrc/mlp_generic.h)"""
    return min(64, max(1, total // 8192))


def instances(cfg, total):
    """(tile of a hidden layer's forward / input-gradient product, splits of the weight gradients, tile of a hidden layer's
    weight-gradient product, k_chunk of the weight gradients)"""
    w = cfg['points_net_width']
    sp = wgrad_splits(total)
    return gemm_tile(total, w, 0), sp, gemm_tile(w, w, sp), -(-total // sp)


# (shape index, rays, samples, rays per part): 512 wide at 32 768 samples, 171 x 192 = 32 832 (a multiple of 64, not of 128,
# on the 128 tile), 256 wide at 65 536
THRESHOLD_CASES = [(0, 128, 256, 32), (0, 171, 192, 57), (5, 256, 256, 32)]


def whole_and_parts(cfg, sd, inputs, grads_in, prec, per_part, bf16):
    n, s = inputs[3].shape
    total = n * s
    tile, splits, wtile, k_chunk = instances(cfg, total)
    part = per_part * s
    p_tile, p_splits, p_wtile, _ = instances(cfg, part)
    assert tile == 128 and splits >= 2, (tile, splits)             # the whole call: 128 x 128 tiles, split-K
    assert p_tile == 64 and p_splits == 1 and p_wtile == 64        # every part: below both thresholds
    mlp, shapes = packed(cfg, sd)
    dev = [t.to(DEV) for t in inputs]
    gs, gc = grads_in[0].to(DEV), grads_in[1].to(DEV)
    sigma_eval, rgb_eval = mlp.forward(*dev, prec)
    sigma, rgb, saved = mlp.forward_train(*dev, prec)
    assert torch.equal(sigma, sigma_eval) and torch.equal(rgb, rgb_eval)
    whole = mlp.backward(saved, sigma, rgb, gs, gc, shapes, prec)
    parts = [torch.zeros_like(g) for g in whole]
    for lo in range(0, n, per_part):
        cut = slice(lo, lo + per_part)
        piece = [t[cut].contiguous() for t in dev]
        sg, cl, sv = mlp.forward_train(*piece, prec)
        # each sample's arithmetic does not depend on the call: both tiles chain k in the same order (mlp_generic_walk.h:27-30)
        assert torch.equal(sg, sigma[cut]) and torch.equal(cl, rgb[cut])
        for acc, g in zip(parts, mlp.backward(sv, sg, cl, gs[cut].contiguous(), gc[cut].contiguous(), shapes, prec)):
            acc += g
    return mlp, shapes, (sigma, rgb, saved), whole, parts, (tile, splits, wtile, k_chunk, part)


def summation_gate(cfg, sd, saved, sigma, rgb, grads_in, whole, parts, total, k_chunk, splits, part, bf16, tag):
    """|whole - parts| per element within the summation bound of the two orders, from the float64 |dZ|^T |X| of the kernel's saved
    operands, and within 1e-4 of each tensor's largest entry."""
    mode = rr.MODES['layered_bf16'] if bf16 else rr.EXACT
    dec = decode_layered(saved, cfg, total, bf16)
    recs = layered_records(sd, cfg, dec, mode)
    if bf16:
        use, eq = check_layers(recs, 'bf16', tag)
        util.observe(f'rounding/{tag}/layers', f'worst |err| / bound {use:.2f} [1], worst bit-equal fraction {eq:.4f} [{BIT_EQUAL_MIN}]')
    else:
        use, _ = check_layers(recs, 'fp32', tag)
        util.observe(f'rounding/{tag}/layers', f'worst |err| / bound {use:.2f} [1]')
    ops_ = {}
    want = reference_grads(sd, cfg, recs, sigma, rgb, grads_in[0], grads_in[1], mode, ops_)
    names = synth.abi_param_list({k: k for k in sd})
    chain = (k_chunk + splits) + (part + total // part)          # the whole call's chain + reduce, a part's chain + the sum of parts
    worst_use, worst_rel = 0.0, 0.0
    for name, a, b in zip(names, whole, parts):
        layer, kind = name.rsplit('.', 1)
        dz, x, dzb = ops_[layer]
        mag = dz.abs().t() @ x.abs() if kind == 'weight' else dzb.abs().sum(0)
        bound = chain * 2.0 ** -24 * mag + 2.0 ** -126
        diff = (a.cpu().double() - b.cpu().double()).abs()
        worst_use = max(worst_use, float((diff / bound).max()))
        if float(b.abs().max()) > 0:
            worst_rel = max(worst_rel, rel_to_max(a, b))
    util.observe(f'rounding/{tag}/whole_vs_parts', f'worst |whole - parts| / summation bound {worst_use:.2f} [1], '
                 f'{worst_rel:.1e} of the largest entry [{WHOLE_VS_PARTS}]')
    assert worst_use <= 1.0 and worst_rel <= WHOLE_VS_PARTS
    if bf16:
        compare_grads(whole, want, names, f'{tag}/gradients')


@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
@pytest.mark.parametrize('index,n,s,per_part', THRESHOLD_CASES)
def test_layered_whole_call_on_the_large_tiles_equals_its_parts(index, n, s, per_part, precision):
    """2d: a call on the 128 x 128 tile (forward, input gradients) with split-K >= 2 (weight gradients) against the sum over parts
    that run the 64 x 64 tile unsplit; plus 2a and 2c on the whole call."""
    bf16 = precision == 'bf16'
    cfg, sd, inputs, grads_in = case(index, n, s)
    mlp, shapes, (sigma, rgb, saved), whole, parts, (tile, splits, wtile, k_chunk, part) = whole_and_parts(
        cfg, sd, inputs, grads_in, P[precision], per_part, bf16)
    tag = f'layered_{precision}/{index}/{n}x{s}'
    util.observe(f'rounding/{tag}/instances', f'whole: tile {tile}, {splits} splits of {k_chunk}; parts of {part}: tile 64, 1 split')
    summation_gate(cfg, sd, saved, sigma, rgb, grads_in, whole, parts, n * s, k_chunk, splits, part, bf16, tag)


def f32_wgrad_instance(cfg, in_dim, total):
    """Which fp32 kernel launch_gemm (csrc/mlp_generic.hip:526-546) runs for a layer's weight gradient dW = dZ^T X: A = dZ along m
    (a_rs 1, a_cs = the dZ row = width), B = X along n (b_cs 1, b_rs = the activation row, a multiple of four floats, every block
    16-byte aligned).  k_chunk does not enter: it only qualifies the operands staged along k, which this product has none of."""
    w = cfg['points_net_width']
    sp = wgrad_splits(total)
    if gemm_tile(w, in_dim, sp) != 128:
        return 'gemm_kernel<64, 64>'
    a_along_m, b_along_n = w % 4 == 0, in_dim % 4 == 0
    return 'gemm_vec_kernel<128, 128, 2, 2>' if a_along_m and b_along_n else 'gemm_kernel<128, 128>'


# (rays, samples, rays per part): 262 144 samples, 32 splits of 8192
WGRAD_CASES = [('fp32', 1024, 256, 32), ('bf16', 1024, 256, 32)]


@pytest.mark.parametrize('precision,n,s,per_part', WGRAD_CASES)
def test_layered_weight_gradient_on_the_large_tile_equals_its_parts(precision, n, s, per_part):
    """2d: the weight-gradient product's 128 x 128 tile (512 wide: splits >= 32) against the sum over unsplit 64-tile parts.  In
    fp32 both 128-tile instances of that product run: the 16-byte one for the 512-wide inputs, the scalar one for the skip layer's
    575 = 63 + 512 columns."""
    cfg, sd, inputs, grads_in = case(0, n, s)
    total = n * s
    _, splits, wtile, k_chunk = instances(cfg, total)
    assert wtile == 128 and splits >= 32
    if precision == 'fp32':
        p = plan_of(cfg)
        kernels = {f32_wgrad_instance(cfg, p['pts_in'] + p['width'] if l == 5 else p['width'], total) for l in range(1, p['depth'])}
        assert kernels == {'gemm_vec_kernel<128, 128, 2, 2>', 'gemm_kernel<128, 128>'}, kernels
    mlp, shapes, _, whole, parts, _ = whole_and_parts(cfg, sd, inputs, grads_in, P[precision], per_part, precision == 'bf16')
    worst = max(rel_to_max(a, b) for a, b in zip(whole, parts) if float(b.abs().max()) > 0)
    util.observe(f'rounding/layered_{precision}/0/{n}x{s}/whole_vs_parts',
                 f'{splits} splits of {k_chunk}: {worst:.1e} of the largest entry [{WHOLE_VS_PARTS}]')
    assert worst <= WHOLE_VS_PARTS


# ------------------------------------------------------------------------------------------------------ e: ragged sweeps
SWEEP = list(range(8))


def fuzz_case(case_):
    """The seeded case `case_` of tests/test_gpu_fuzz.py::test_fused_mlp_random_shapes (the same draws, in the same order), plus
    upstream gradients drawn after them."""
    rng = numpy.random.RandomState(1000 + case_)
    layout = ['main', 'ptsaug', 'viewsaug'][case_ % 3]
    depth, width, vwidth = [(8, 256, 128), (4, 128, 64), (2, 128, 64), (6, 256, 128), (1, 256, 128)][case_ % 5]
    cfg = synth.mlp_config(64, depth=depth, width=width, views_width=vwidth, **LAYOUTS[layout])
    sd = synth.synth_state_dict(util.mlp_param_shapes(cfg), 200 + case_, float(rng.choice([1.0, 30.0, 200.0])), float(rng.uniform(-3, 3)))
    n, s = int(rng.randint(1, 90)), int(rng.choice([1, 2, 31, 33, 64, 127, 129, 192]))
    spread = float(rng.choice([1.0, 6.0]))
    o = torch.from_numpy(rng.uniform(-spread, spread, (n, 3)).astype(numpy.float32))
    d = torch.from_numpy(rng.uniform(-1, 1, (n, 3)).astype(numpy.float32))
    v = d / d.norm(dim=1, keepdim=True)
    z = torch.from_numpy(numpy.sort(rng.uniform(0, 1, (n, s)).astype(numpy.float32), axis=1))
    noise = torch.from_numpy(rng.standard_normal((n, s, 1)).astype(numpy.float32)) if case_ % 2 else torch.zeros(n, s, 1)
    g = (torch.from_numpy(rng.standard_normal((n, s, 1)).astype(numpy.float32)),
         torch.from_numpy(rng.standard_normal((n, s, 3)).astype(numpy.float32)))
    return cfg, sd, (o, d, v, z, noise), g, f'{layout}/{depth}x{width}/{n}x{s}'


@pytest.mark.parametrize('case_', range(10))
def test_fused_16bit_modes_on_the_fuzz_cases(case_):
    """2e: the seeded ragged cases of test_gpu_fuzz.py in the 16-bit modes: in 'f16' and 'bf16' every layer (2a), sigma / rgb
    from the kernel's own saved inputs of the heads (2b) and the gradients with the kernel's own masks (2c); the s8 modes' forward
    is theirs bit for bit.  (From scratch, single midpoint flips carried through the 256-wide world-space case 4 moved f16 rgb by
    1.4e-5, above 2b's 1e-5, with every layer within its bound: the from-scratch comparison is made on the fixed cases above.)"""
    cfg, sd, inputs, grads_in, name = fuzz_case(case_)
    mlp, _ = packed(cfg, sd)
    dev = [t.to(DEV) for t in inputs]
    for precision in ('f16', 'bf16'):
        fused_layers_and_gradients(cfg, sd, inputs, grads_in, precision, f'fuzz/{case_}/{name}/{precision}')
        sigma, rgb, _ = mlp.forward_train(*dev, P[precision])
        s8_sigma, s8_rgb, _ = mlp.forward_train(*dev, P[precision + 's8'])
        assert torch.equal(s8_sigma, sigma) and torch.equal(s8_rgb, rgb), precision


@pytest.mark.parametrize('case_', SWEEP)
def test_layered_bf16_on_random_shapes(case_):
    """Widths that are not multiples of 8 (element-by-element staging), depth 1-9 with and without the skip layer (5 is no
    reference shape), views depth 1-3, both augmentation layouts: 2a and 2c.  2b is left to 2a's check of the two head layers here:
    from scratch, single midpoint flips carried through up to nine narrow layers moved rgb by up to 1.3e-4 (a 75-wide
    points-augmentation MLP, every layer within its bound and 99.99 % bit-equal) -- above 2b's 5e-5, and not a kernel fault."""
    rng = numpy.random.RandomState(4000 + case_)
    layout = ['main', 'ptsaug', 'viewsaug', 'main'][case_ % 4]
    depth = [1, 9, 3, 6, 2, 7, 4, 8][case_]
    width = int(rng.choice([37, 75, 131, 203]))
    vwidth, vdepth = int(rng.choice([19, 45, 70])), int(rng.randint(1, 4))
    cfg = synth.mlp_config(64, depth=depth, width=width, views_width=vwidth, views_depth=vdepth, **LAYOUTS[layout])
    sd = synth.synth_state_dict(util.mlp_param_shapes(cfg), 500 + case_, 30.0, 0.5)
    n, s = int(rng.randint(1, 40)), int(rng.choice([1, 31, 33, 129]))
    o = torch.from_numpy(rng.uniform(-1, 1, (n, 3)).astype(numpy.float32))
    d = torch.from_numpy(rng.uniform(-1, 1, (n, 3)).astype(numpy.float32))
    v = d / d.norm(dim=1, keepdim=True)
    z = torch.from_numpy(numpy.sort(rng.uniform(0, 1, (n, s)).astype(numpy.float32), axis=1))
    noise = torch.from_numpy(rng.standard_normal((n, s, 1)).astype(numpy.float32))
    grads_in = (torch.from_numpy(rng.standard_normal((n, s, 1)).astype(numpy.float32)),
                torch.from_numpy(rng.standard_normal((n, s, 3)).astype(numpy.float32)))
    layered_case_checks(cfg, sd, (o, d, v, z, noise), grads_in, f'layered_sweep/{case_}/{layout}/{depth}x{width}x{vwidth}x{vdepth}',
                        outputs=False)


# --------------------------------------------------------------------------------------------------------------- f: edges
def test_layered_bf16_with_a_hidden_unit_of_1e5():
    cfg, sd, inputs, grads_in = case(1, 5, 37)
    sd = dict(sd)
    w = sd['pts_linears.1.weight'].copy()
    w[3] *= 2e5                               # unit 3 of h_2 reaches ~1e5
    sd['pts_linears.1.weight'] = w
    _, _, _, _, recs = layered_case_checks(cfg, sd, inputs, grads_in, 'edge/layered_bf16/unit_1e5', outputs=False)
    assert float(recs[1]['out'][:, 3].max()) > 3e4


def test_layered_bf16_with_an_upstream_gradient_zero_on_most_samples():
    cfg, sd, inputs, (g_sigma, g_rgb) = case(0, 5, 37)
    keep = (torch.arange(5 * 37).reshape(5, 37, 1) % 23 == 0).float()
    layered_case_checks(cfg, sd, inputs, (g_sigma * keep, g_rgb * keep), 'edge/layered_bf16/sparse_upstream', layers=False,
                        outputs=False)


@pytest.mark.parametrize('precision', ['f16', 'bf16'])
def test_fused_activations_in_the_fp16_subnormal_range(precision):
    """2f: layer 1 scaled down so that h_2 and what follows lie below fp16's normal range (6.1e-5): every layer from the kernel's
    saved input, subnormal results included (rounding_ref rounds with subnormals, as v_cvt_pk_f16_f32 does)."""
    cfg, sd, inputs, grads_in = fused_case('main', (4, 128, 64))
    sd = dict(sd)
    sd['pts_linears.1.weight'] = sd['pts_linears.1.weight'] * 2e-5
    sd['pts_linears.1.bias'] = sd['pts_linears.1.bias'] * 2e-5
    recs = fused_layers_and_gradients(cfg, sd, inputs, grads_in, precision, f'edge/fused/{precision}/subnormal', gradients=False)
    h2 = recs[1]['out']
    sub = (h2 > 0) & (h2 < 2.0 ** -14)
    assert float(sub.double().mean()) > 0.1, float(sub.double().mean())


@pytest.mark.parametrize('precision', ['f16s8', 'bf16s8'])
def test_s8_trunk_above_the_fp8_clamp(precision):
    """2f: eight units of h_2 held at constants in (250, 900) -- on both sides of the clamp at 448, and all above 224 -- and eight
    in e4m3's subnormal range 2^-9 .. 2^-6.  The s8 mode differs from its 16-bit mode ONLY in the X operand of the trunk weight
    gradients (the chain, and so every dZ, is the same), so the kernels' g_s8 - g_16 of the weight gradient that reads h_2 is
    dZ^T (e4m3(min(h_2, 448)) - h_2); it is compared with the same difference of the emulated backward."""
    cfg, sd, inputs, (g_sigma, g_rgb) = fused_case('main', (8, 256, 128))
    sd = dict(sd)
    w, b = sd['pts_linears.1.weight'].copy(), sd['pts_linears.1.bias'].copy()
    w[:16] = 0.0
    b[:8] = numpy.linspace(250.0, 900.0, 8)
    b[8:16] = numpy.linspace(2.0 ** -9, 2.0 ** -6, 10)[1:9]
    sd['pts_linears.1.weight'], sd['pts_linears.1.bias'] = w, b
    base = precision[:-2]
    modes = {q: rr.MODES[FUSED_MODES[q]] for q in (precision, base)}
    ref = emulated(cfg, sd, inputs, modes[precision])
    mlp, shapes = packed(cfg, sd)
    dev = [t.to(DEV) for t in inputs]
    name = 'pts_linears.2.weight'
    index = synth.abi_param_list({k: k for k in sd}).index(name)
    got, want = {}, {}
    for q, mode in modes.items():
        sigma, rgb, saved = mlp.forward_train(*dev, P[q])
        got[q] = mlp.backward(saved, sigma, rgb, g_sigma.to(DEV), g_rgb.to(DEV), shapes, P[q])[index]
        dout, dvout = rr.heads_backward(sigma.cpu(), rgb.cpu(), g_sigma, g_rgb, True, exact=False)
        want[q] = rr.backward(rr.mlp_params64(sd), cfg, ref['layers'], dout, dvout, mode)[name]
    delta_got, delta_want = got[precision] - got[base], want[precision] - want[base]
    err = rel_l2(delta_got, delta_want)
    util.observe(f'rounding/edge/{precision}/clamp', f'(g_s8 - g_16) of {name}: rel L2 {err:.1e} [{S8_DELTA_L2}]')
    assert float(delta_want.abs().max()) > 0 and err <= S8_DELTA_L2
