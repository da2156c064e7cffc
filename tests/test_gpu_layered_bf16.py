"""hip_precision 'bf16' / 'bf16s8' on the layered MLP path (csrc/mlp_generic_bf16.hip): every MLP shape the fused kernels are not
built for, on bf16 operands (v_mfma_f32_32x32x16_bf16, fp32 accumulation and master weights, bf16 activations and layer
gradients, fp32 heads).  Tolerances are the fused bf16 kernels' (tests/test_gpu_bf16.py); what each test observes is printed in
pytest's summary.  Exact properties are tested exactly: bit-reproducible results, the keeping and the inference forward giving the
same bits, 'bf16s8' = 'bf16', linearity of the backward in the upstream gradient, a large call equal to its parts."""
import ctypes

import pytest
import torch

from oracle import nerf_oracle as oracle
from simplenerf_amd import _lib, harness, ops, optim, synth
from simplenerf_amd.data_preprocessors.BatchAssembler01 import BatchAssembler
from simplenerf_amd.loss_functions.LossComputer01 import LossComputer
from tests import util
from tests.test_gpu_f16 import synthetic_model
from tests.test_gpu_generic import SHAPES, case
from tests.test_gpu_grads import rel_l2, rel_to_max

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
BF16 = ops.PRECISIONS['bf16']
BF16S8 = ops.PRECISIONS['bf16s8']
GUARD = 1 << 20            # floats on either side of a scratch buffer (as tests/test_gpu_workspace_bounds.py)
PATTERN = 0x7fa5a5a5       # a NaN payload no kernel produces


def packed(cfg, sd):
    plist = synth.abi_param_list({k: torch.from_numpy(a).to(DEV) for k, a in sd.items()})
    mlp = ops.PackedMlp(cfg, DEV)
    mlp.pack(plist)
    return mlp, [tuple(p.shape) for p in plist]


# sigma relative L-inf against the fp32 oracle: the fused bf16 kernels' 2e-2, except for shape 2 (6 x 96 / 3 x 48), where the mode's
# own rounding -- weights and every layer input rounded to bf16, fp32 sums, emulated on the CPU -- already gives 4.0e-2 (what the
# kernels produce, to three digits; the other shapes: 4.9e-3 .. 1.1e-2, also as emulated)
SIGMA_BOUND = {2: 6e-2}


@pytest.mark.parametrize('index', range(len(SHAPES)))
def test_layered_bf16_mlp_against_the_oracle(index):
    cfg, sd, inputs, (g_sigma, g_rgb) = case(index, 9, 64)
    o, d, v, z, noise = inputs
    params = {k: torch.from_numpy(a).clone().requires_grad_(True) for k, a in sd.items()}
    ref = oracle.run_mlp(params, '', cfg, oracle.ray_points(o, d, z), v if cfg['use_view_dirs'] else None, None, noise)
    ((ref['sigma'] * g_sigma).sum() + (ref['rgb'] * g_rgb).sum()).backward()
    mlp, shapes = packed(cfg, sd)
    dev = [t.to(DEV) for t in inputs]
    sigma_eval, rgb_eval = mlp.forward(*dev, BF16)
    sigma, rgb, saved = mlp.forward_train(*dev, BF16)
    assert torch.equal(sigma, sigma_eval) and torch.equal(rgb, rgb_eval)          # the same kernels, with and without keeping
    e_sigma, e_rgb = util.rel_linf(sigma, ref['sigma']), util.linf(rgb, ref['rgb'])
    grads = mlp.backward(saved, sigma, rgb, g_sigma.to(DEV), g_rgb.to(DEV), shapes, BF16)
    again = mlp.backward(saved, sigma, rgb, g_sigma.to(DEV), g_rgb.to(DEV), shapes, BF16)
    names = synth.abi_param_list({k: k for k in sd})
    worst = 0.0
    for name, got, twice in zip(names, grads, again):
        assert torch.equal(got, twice), name                                       # fixed-order reductions
        want = params[name].grad
        assert got.shape == want.shape and bool(torch.isfinite(got).all()), name
        if float(want.abs().max()) > 0:
            worst = max(worst, rel_l2(got, want))
    bound = SIGMA_BOUND.get(index, 2e-2)
    util.observe(f'layered_bf16/{index}', f'sigma rel {e_sigma:.1e} [{bound}], rgb {e_rgb:.1e} [5e-4], worst gradient rel L2 {worst:.3f} [0.25]')
    assert e_sigma < bound and e_rgb < 5e-4, (e_sigma, e_rgb)
    assert worst < 0.25, worst


def test_bf16s8_is_bf16_bit_for_bit_on_a_layered_shape():
    cfg, sd, inputs, (g_sigma, g_rgb) = case(0, 5, 37)
    mlp, shapes = packed(cfg, sd)
    dev = [t.to(DEV) for t in inputs]
    outs = {}
    for prec in (BF16, BF16S8):
        sigma_eval, rgb_eval = mlp.forward(*dev, prec)
        sigma, rgb, saved = mlp.forward_train(*dev, prec)
        grads = mlp.backward(saved, sigma, rgb, g_sigma.to(DEV), g_rgb.to(DEV), shapes, prec)
        outs[prec] = [sigma_eval, rgb_eval, sigma, rgb] + grads
    assert all(torch.equal(a, b) for a, b in zip(outs[BF16], outs[BF16S8]))


def test_layered_bf16_backward_is_linear_in_the_loss_scale():
    """dZ is rounded to bf16 and bf16 keeps fp32's exponent: scaling the upstream gradient by 2^-30 scales every rounding step
    exactly, so every parameter gradient scales by exactly 2^-30."""
    cfg, sd, inputs, (g_sigma, g_rgb) = case(0, 5, 37)
    mlp, shapes = packed(cfg, sd)
    sigma, rgb, saved = mlp.forward_train(*[t.to(DEV) for t in inputs], BF16)
    ref = mlp.backward(saved, sigma, rgb, g_sigma.to(DEV), g_rgb.to(DEV), shapes, BF16)
    k = 2.0 ** -30
    small = mlp.backward(saved, sigma, rgb, (g_sigma * k).to(DEV), (g_rgb * k).to(DEV), shapes, BF16)
    for a, b in zip(ref, small):
        assert torch.equal(a * k, b)


@pytest.mark.parametrize('index', [0, 1, 4])
def test_layered_bf16_large_call_equals_its_parts(index):
    """13 440 samples (70 rays x 192): the inference forward equals that of ten 7-ray parts bit for bit (each sample's arithmetic
    does not depend on the call), and the parameter gradients equal the sum over the parts' gradients up to the order of the
    fp32 sums over the samples (split-K partials, bias sums: 1e-4 of each tensor's largest entry)."""
    cfg, sd, inputs, (g_sigma, g_rgb) = case(index, 70, 192)
    mlp, shapes = packed(cfg, sd)
    dev = [t.to(DEV) for t in inputs]
    gs, gc = g_sigma.to(DEV), g_rgb.to(DEV)
    sigma_eval, rgb_eval = mlp.forward(*dev, BF16)
    sigma, rgb, saved = mlp.forward_train(*dev, BF16)
    assert torch.equal(sigma, sigma_eval) and torch.equal(rgb, rgb_eval)
    whole = mlp.backward(saved, sigma, rgb, gs, gc, shapes, BF16)
    parts = [torch.zeros_like(g) for g in whole]
    for lo in range(0, 70, 7):
        cut = slice(lo, lo + 7)
        piece = [t[cut].contiguous() for t in dev]
        se, ce = mlp.forward(*piece, BF16)
        assert torch.equal(se, sigma[cut]) and torch.equal(ce, rgb[cut])
        sg, cl, sv = mlp.forward_train(*piece, BF16)
        assert torch.equal(sg, sigma[cut]) and torch.equal(cl, rgb[cut])
        for acc, g in zip(parts, mlp.backward(sv, sg, cl, gs[cut].contiguous(), gc[cut].contiguous(), shapes, BF16)):
            acc += g
    worst = max(rel_to_max(a, b) for a, b in zip(whole, parts) if float(b.abs().max()) > 0)
    util.observe(f'layered_bf16/{index}/70x192', f'gradients of the whole call vs the sum over ten parts: {worst:.1e} of the largest entry [1e-4]')
    assert worst < 1e-4


@pytest.mark.parametrize('index', [0, 1, 2, 4])
@pytest.mark.parametrize('n,s', [(7, 45), (300, 131)])
def test_layered_bf16_scratch_stays_inside_the_reported_sizes(index, n, s):
    """The bf16 activation matrix + heads block inside snerf_mlp_saved_floats(), the backward's bf16 dZ buffers, head gradients
    and partial sums inside snerf_mlp_backward_workspace_floats(): guard regions on either side stay untouched."""
    cfg, sd, inputs, (g_sigma, g_rgb) = case(index, n, s)
    mlp, shapes = packed(cfg, sd)
    dev = [t.to(DEV) for t in inputs]
    ref_sigma, ref_rgb, ref_saved = mlp.forward_train(*dev, BF16)
    saved_need = ref_saved.numel()
    arena = torch.full((GUARD + saved_need + GUARD,), PATTERN, dtype=torch.int32, device=DEV)
    saved = arena[GUARD:GUARD + saved_need].view(torch.float32)
    lib = _lib.load()
    sigma, rgb = torch.empty_like(ref_sigma), torch.empty_like(ref_rgb)
    o, d, v, z, noise = dev
    st = lib.snerf_mlp_forward_train(ctypes.byref(mlp.desc), ops._ptr(mlp.buffer), ops._ptr(o), ops._ptr(d),
                                     ops._ptr(v if cfg['use_view_dirs'] else None), ops._ptr(z), n, s, ops._ptr(noise),
                                     ops._ptr(sigma), ops._ptr(rgb), ops._ptr(saved), BF16, ops._stream())
    _lib.check(st, 'snerf_mlp_forward_train')
    torch.cuda.synchronize()
    assert torch.equal(sigma, ref_sigma) and torch.equal(rgb, ref_rgb)
    assert (arena[:GUARD] != PATTERN).sum() == 0 and (arena[GUARD + saved_need:] != PATTERN).sum() == 0
    need = mlp.backward_workspace_floats(n, s)
    work_arena = torch.full((GUARD + need + GUARD,), PATTERN, dtype=torch.int32, device=DEV)
    work = work_arena[GUARD:GUARD + need].view(torch.float32)
    grads = mlp.backward(saved, sigma, rgb, g_sigma.to(DEV), g_rgb.to(DEV), shapes, BF16, work=work)
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(g).all()) for g in grads)
    before = (work_arena[:GUARD] != PATTERN).nonzero()
    after = (work_arena[GUARD + need:] != PATTERN).nonzero()
    assert before.numel() == 0, f'{before.numel()} words written in front of the workspace'
    assert after.numel() == 0, f'{after.numel()} words written behind the workspace of {need} floats'


@pytest.mark.parametrize('precision', ['f16', 'f16s8', 'f16x3'])
def test_the_fp16_modes_stay_refused_on_layered_shapes(precision):
    cfg, sd, inputs, (g_sigma, g_rgb) = case(1)
    mlp, shapes = packed(cfg, sd)
    dev = [t.to(DEV) for t in inputs]
    prec = ops.PRECISIONS[precision]
    with pytest.raises(Exception, match="'fp32' or 'bf16'"):
        mlp.forward(*dev, prec)
    with pytest.raises(Exception, match="'fp32' or 'bf16'"):
        mlp.forward_train(*dev, prec)
    sigma, rgb, saved = mlp.forward_train(*dev, BF16)
    with pytest.raises(Exception, match="'fp32' or 'bf16'"):
        mlp.backward(saved, sigma, rgb, g_sigma.to(DEV), g_rgb.to(DEV), shapes, prec)


def layered_configs(base, width, views_width, views_depth):
    for key in ('coarse_mlp', 'fine_mlp'):
        base['model'][key].update(points_net_width=width, views_net_width=views_width, views_net_depth=views_depth)
    return base


LAYERED = [(512, 256, 1), (64, 64, 2)]


@pytest.mark.parametrize('width,views_width,views_depth', LAYERED)
def test_layered_bf16_render_close_to_fp32(width, views_width, views_depth):
    cfg = layered_configs(synth.make_configs('config2'), width, views_width, views_depth)
    batch = harness.frame_batch(synth.camera('fern', 0), True, DEV, 95000, 2048)
    with torch.no_grad():
        ref = synthetic_model(cfg, 'fp32').eval()(batch)
        got = synthetic_model(cfg, 'bf16').eval()(batch)
        again = synthetic_model(cfg, 'bf16').eval()(batch)
    assert all(torch.equal(got[k], again[k]) for k in got)
    worst = {k: util.linf(got[k], ref[k]) for k in ('rgb_coarse', 'rgb_fine', 'depth_ndc_coarse', 'depth_ndc_fine')}
    util.observe(f'layered_bf16/render/{width}x{views_width}x{views_depth}',
                 ', '.join(f'{k} {v:.1e}' for k, v in worst.items()) + ' [rgb 4e-3, NDC depth 5e-3]')
    assert worst['rgb_coarse'] < 4e-3 and worst['rgb_fine'] < 4e-3
    assert worst['depth_ndc_coarse'] < 5e-3 and worst['depth_ndc_fine'] < 5e-3


def training_run_configs(precision, width, views_width, views_depth):
    cfg = synth.training_configs(precision, num_rays=1024, num_sparse=256)
    cfg['sub_batch_size'] = 1280
    cfg['losses'] = synth.loss_configs(iter_weighted=False)
    model_cfg = cfg['model']
    for key in [k for k in model_cfg if k.endswith('_mlp')]:
        model_cfg[key].update(points_net_width=width, views_net_width=views_width, views_net_depth=views_depth)
    for aug in ('points_augmentation', 'views_augmentation'):
        for key in [k for k in model_cfg.get(aug, {}) if k.endswith('_mlp')]:
            model_cfg[aug][key].update(points_net_width=width, views_net_width=views_width, views_net_depth=views_depth)
    return cfg


@pytest.mark.parametrize('width,views_width,views_depth', LAYERED)
def test_layered_bf16_training_batch_close_to_fp32(width, views_width, views_depth):
    """One reference-shaped training batch (four MLPs, nine losses) in 'bf16' against 'fp32', bit-reproducible."""
    def run(precision):
        cfg = training_run_configs(precision, width, views_width, views_depth)
        model = synthetic_model(cfg, precision).train()
        batch = BatchAssembler(cfg, synth.training_scene(0, 3, 96, 128, sparse_fraction=0.02), DEV).get_next_batch(0)
        losses = LossComputer(cfg)
        out = model(batch)
        terms = losses.compute_losses(batch, out)
        terms['TotalLoss'].backward()
        values = {k: float((v['loss_value'] if isinstance(v, dict) else v).detach()) for k, v in terms.items()}
        return values, {n: p.grad.clone() for n, p in model.named_parameters()}

    ref_loss, ref_grads = run('fp32')
    got_loss, got_grads = run('bf16')
    again_loss, again_grads = run('bf16')
    assert got_loss == again_loss and all(torch.equal(got_grads[k], again_grads[k]) for k in got_grads)
    worst_loss = max(abs(got_loss[k] - v) / max(abs(v), 1e-6) for k, v in ref_loss.items())
    worst_grad = max(rel_l2(got_grads[k], ref_grads[k]) for k in ref_grads)
    util.observe(f'layered_bf16/training_batch/{width}x{views_width}x{views_depth}',
                 f'worst loss value rel {worst_loss:.1e} [4e-2], worst gradient rel L2 {worst_grad:.3f} [0.20]')
    assert worst_loss <= 4e-2 and worst_grad <= 0.20


def test_graphed_training_pass_in_bf16_on_a_layered_shape_equals_eager():
    """harness.GraphedTrainStep (one captured HIP graph: re-pack, forwards, losses, backward) on a 64-wide, views-depth-2 model in
    'bf16' against the same pass run eagerly: identical losses and bit-identical gradients on the capture and on replays.  (The
    layered training path takes its scratch from the caller; only the inference entry point's scratch block must exist before a
    capture, and this pass does not use it.)"""
    from simplenerf_amd.models.ModelFactory import get_model
    cfg = synth.training_configs('bf16', num_rays=192, num_sparse=64)
    cfg['losses'] = synth.loss_configs(iter_weighted=False)
    for key in [k for k in cfg['model'] if k.endswith('_mlp')]:
        cfg['model'][key].update(points_net_width=64, views_net_width=64, views_net_depth=2)
    scene = synth.training_scene(0, 3, 48, 64, sparse_fraction=0.05)
    models = []
    for _ in range(2):
        m = get_model(cfg, None)
        shapes = {k: tuple(v.shape) for k, v in m.state_dict().items()}
        m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.synth_state_dict(shapes, 9, 200.0, 8.0).items()})
        models.append(m.to(DEV).train())
    eager, graphed = models
    batcher = BatchAssembler(cfg, scene, DEV)
    losses = LossComputer(cfg)
    step = harness.GraphedTrainStep(graphed, losses, batcher.get_next_batch(0))
    opt_e, opt_g = optim.Adam(list(eager.parameters()), lr=1e-3), optim.Adam(list(graphed.parameters()), lr=1e-3)
    for it in range(3):
        batch = batcher.get_next_batch(it)
        eager.set_random_draws(eager.draw_training_randomness(256, 0, DEV))
        piece = dict(batch)
        piece['common_data'] = dict(batch['common_data'])
        opt_e.zero_grad(set_to_none=True)
        ref = losses.compute_losses(piece, eager(piece))
        ref['TotalLoss'].backward()
        totals = step(batch)
        assert float(totals['TotalLoss']) == float(ref['TotalLoss'].detach()), it
        for (name, a), b in zip(eager.named_parameters(), graphed.parameters()):
            assert torch.equal(a.grad, b.grad), (it, name)
        opt_e.step()
        opt_g.step()
    for a, b in zip(eager.parameters(), graphed.parameters()):
        assert torch.equal(a, b)
