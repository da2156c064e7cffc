"""The plain (01) depth losses, DenseDepthMSE01 and the dense-depth batch keys on the GPU: against fixtures made by running
the reference's own classes (tools/make_golden_losses01.py), against a float64 evaluation written out here, and the exact
properties of the two-sided loss term (include/simplenerf_train.h, ``snerf_loss_term.d_target``)."""
import copy

import numpy
import pytest
import torch

from simplenerf_amd import ops, synth
from simplenerf_amd.data_preprocessors.BatchAssembler01 import BatchAssembler
from simplenerf_amd.loss_functions.LossComputer01 import LossComputer
from tests import util

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
REL = 5e-6   # the loss tolerance of tests/test_gpu_losses.py: fp32 sums in a different (fixed) order than torch's
PLAIN = {'PointsAugmentationDepthLoss01': ('depth_{}', 'points_augmentation_depth_{}'),
         'ViewsAugmentationDepthLoss01': ('depth_{}', 'views_augmentation_depth_{}')}


def case_inputs(name, device=DEV):
    """(configs, input_dict, output_dict) of a ``synth.LOSS01_CASES`` entry; ``common_data`` replicated once, as the loader does."""
    configs, scene, batch, keys = synth.loss01_case(name)
    t = lambda a: torch.from_numpy(numpy.ascontiguousarray(a)).to(device)
    inp = {'iter_num': synth.LOSS01_CASES[name]['iter_num'], 'rays_o': t(batch['rays_o']), 'rays_d': t(batch['rays_d']),
           'pixel_id': t(batch['pixel_id']), 'target_rgb': t(batch['target_rgb']), 'indices_mask_nerf': t(batch['indices_mask_nerf']),
           'indices_mask_sparse_depth': t(batch['indices_mask_sparse_depth']), 'sparse_depth_values': t(batch['sparse_depth_values']),
           'common_data': {'poses': t(scene['poses'])[None], 'images': t(scene['images'])[None],
                           'intrinsics': t(scene['intrinsics'])[None], 'resolution': scene['resolution']}}
    if 'dense_depth_values' in batch:
        inp['dense_depth_values'] = t(batch['dense_depth_values'])
    out = {k: t(batch[k]).clone().requires_grad_(True) for k in keys}
    return configs, inp, out


def float64_value(name, configs, inp, out):
    """The reference's formula for one of the four new losses, written out in float64 (mean of squared differences)."""
    model = configs['model']
    d = lambda k: out[k].detach().double()
    if name in PLAIN:
        aug = 'points_augmentation' if name.startswith('Points') else 'views_augmentation'
        return sum(float(((d(PLAIN[name][0].format(level)) - d(PLAIN[name][1].format(level))) ** 2).mean())
                   for level in ('coarse', 'fine') if f'{level}_mlp' in model and f'{level}_mlp' in model[aug])
    if name == 'CoarseFineConsistencyLoss01':
        both = 'coarse_mlp' in model and 'fine_mlp' in model
        return float(((d('depth_coarse') - d('depth_fine')) ** 2).mean()) if both else 0.0
    mask = inp['indices_mask_nerf']
    if not bool(mask.any()):
        return 0.0
    gt = inp['dense_depth_values'][:, 0].double()[mask]
    return sum(float(((d(f'depth_{level}')[mask] - gt) ** 2).mean()) for level in ('coarse', 'fine') if f'{level}_mlp' in model)


@pytest.mark.parametrize('case', list(synth.LOSS01_CASES))
def test_losses01_match_the_reference_classes(case):
    """Every loss value, TotalLoss and dTotalLoss/d(output) of every output key against the fixture the reference's classes
    produced; the four new losses also against float64.  Tolerance: REL of tests/test_gpu_losses.py, gradients relative to
    the tensor's largest entry, as there."""
    g = util.load(f'losses01_{case}.npz')
    configs, inp, out = case_inputs(case)
    losses = LossComputer(configs).compute_losses(inp, out)
    total = float(losses['TotalLoss'].detach())
    print(f"{case}: TotalLoss {total!r} reference {float(g['TotalLoss'])!r}")
    assert total == pytest.approx(float(g['TotalLoss']), rel=REL, abs=1e-9)
    for cfg in configs['losses']:
        name = cfg['name']
        value = float(losses[name]['loss_value'].detach())
        print(f"{case}: {name} {value!r} reference {float(g[f'value_{name}'])!r}")
        assert value == pytest.approx(float(g[f'value_{name}']), rel=REL, abs=1e-9), name
        if name.endswith('Loss01') or name == 'DenseDepthMSE01':
            assert value == pytest.approx(float64_value(name, configs, inp, out), rel=REL, abs=1e-9), name
    losses['TotalLoss'].backward()
    for k in out:
        grad = out[k].grad
        grad = numpy.zeros_like(g[f'grad_{k}']) if grad is None else grad.cpu().numpy()
        scale = max(float(numpy.abs(g[f'grad_{k}']).max()), 1e-12)
        print(f"{case}: grad {k} linf {util.linf(grad, g[f'grad_{k}']):.3e} of {scale:.3e}")
        assert util.linf(grad, g[f'grad_{k}']) <= REL * scale, k
    if case == 'early':       # weight 0: the consistency losses report their value and move nothing
        assert not out['points_augmentation_depth_coarse'].grad[:320].any()
    if case == 'world':       # both operands differentiated: depth_fine's pixel rows are read by CoarseFineConsistencyLoss01 alone
        assert int((out['depth_fine'].grad[:320] != 0).sum()) == 320


@pytest.mark.parametrize('case', ['world', 'dense', 'empty'])
def test_loss_maps01_match_the_reference(case):
    g = util.load(f'losses01_{case}.npz')
    configs, inp, out = case_inputs(case)
    losses = LossComputer(configs).compute_losses(inp, out, return_loss_maps=True)
    seen = set()

    def walk(prefix, maps):
        for key, value in maps.items():
            if isinstance(value, dict):
                walk(f'{prefix}/{key}', value)
            else:
                ref = g[f'{prefix}/{key}']
                assert util.linf(value.detach().cpu().numpy(), ref) <= 1e-6 * max(1.0, float(numpy.abs(ref).max()) if ref.size else 1.0), key
                seen.add(f'{prefix}/{key}')

    for name, entry in losses.items():
        if f'has_maps_{name}' in g:
            assert ('loss_maps' in entry) == bool(g[f'has_maps_{name}']), name
            walk(f'map/{name}', entry.get('loss_maps', {}))
    assert seen == {k for k in g if k.startswith('map/')} and (seen or case == 'empty')
    if case == 'dense':       # no fine MLP: the reference's CoarseFineConsistencyLoss01 returns no maps entry at all
        assert 'loss_maps' not in losses['CoarseFineConsistencyLoss01']
        assert set(losses['PointsAugmentationDepthLoss01']['loss_maps']) == {'PointsAugmentationDepthLoss01'}


def _bits(t):
    return t.contiguous().view(torch.int32)


def test_second_operand_gradient_is_the_bitwise_negation():
    n = 5000
    gen = torch.Generator(device=DEV).manual_seed(3)
    a, b, c, d = (4 + torch.randn((n,), device=DEV, generator=gen) for _ in range(4))
    b[::7] = a[::7]                                              # exact ties: +0 on one side, -0 on the other
    rgb1, rgb2 = torch.rand((n, 3), device=DEV, generator=gen), torch.rand((n, 3), device=DEV, generator=gen)
    keep = torch.rand((n,), device=DEV, generator=gen) < 0.6
    part = keep & (torch.rand((n,), device=DEV, generator=gen) < 0.5)
    terms = [ops.LossTermSpec(a, b, None, None, 0, 0.1, two_sided=True), ops.LossTermSpec(c, d, part, keep, 1, 0.3, two_sided=True),
             ops.LossTermSpec(rgb1, rgb2, keep, keep, 1, 1.0, two_sided=True)]
    values, scales = ops.loss_forward(terms, 2)
    one_sided = [ops.LossTermSpec(t.pred, t.target, t.numerator_mask, t.denominator_mask, t.group, t.weight) for t in terms]
    assert torch.equal(values, ops.loss_forward(one_sided, 2)[0])          # one term, counted once
    up = torch.zeros(6, device=DEV)
    up[5] = 1.0
    grads, target_grads = ops.loss_backward(terms, 2, scales, up, [True] * 3, [True] * 3)
    sign = torch.tensor(-2 ** 31, dtype=torch.int32, device=DEV)
    for i, on in enumerate((torch.ones_like(keep), part, keep)):
        assert torch.equal(_bits(target_grads[i])[on], _bits(grads[i])[on] ^ sign), i
        assert not _bits(target_grads[i])[~on].any() and not _bits(grads[i])[~on].any(), i       # +0 off the mask, both sides
        assert torch.equal(grads[i], ops.loss_backward(one_sided, 2, scales, up, [True] * 3)[i]), i
    assert float(grads[0].abs().max()) > 0 and int((_bits(target_grads[0])[::7] == sign).sum()) == len(a[::7])
    # only the second operand wanted
    only = ops.loss_backward(terms, 2, scales, up, [False] * 3, [True, False, True])
    assert only[0] == [None] * 3 and only[1][1] is None
    assert torch.equal(only[1][0], target_grads[0]) and torch.equal(only[1][2], target_grads[2])
    with pytest.raises(RuntimeError, match='two_sided'):
        ops.loss_backward(one_sided, 2, scales, up, [True] * 3, [True] * 3)


def test_a_tensor_that_is_pred_here_and_target_there_gets_one_summed_buffer():
    """depth_coarse is pred of SparseDepthMSE01 and of the 01 terms, depth_fine is target of CoarseFineConsistencyLoss01 and
    pred of another term: one buffer per tensor holding the sum over both roles, added in table order."""
    n = 3000
    gen = torch.Generator(device=DEV).manual_seed(4)
    coarse, fine, aug, data = (4 + torch.randn((n,), device=DEV, generator=gen) for _ in range(4))
    sd = torch.rand((n,), device=DEV, generator=gen) < 0.2
    terms = [ops.LossTermSpec(fine, data, sd, sd, 0, 0.1), ops.LossTermSpec(coarse, aug, None, None, 1, 0.1, two_sided=True),
             ops.LossTermSpec(coarse, fine, None, None, 2, 0.2, two_sided=True), ops.LossTermSpec(aug, data, sd, sd, 3, 0.5)]
    values, scales = ops.loss_forward(terms, 4)
    up = torch.zeros(9, device=DEV)
    up[8] = 1.0
    grads, tg = ops.loss_backward(terms, 4, scales, up, [True] * 4, [False, True, True, False])
    assert grads[1] is grads[2] and grads[0] is tg[2] and grads[3] is tg[1] and tg[0] is None
    e = lambda x, y: x.double() - y.double()
    cnt = sd.sum().double()
    want_coarse = 0.1 * 2 * e(coarse, aug) / n + 0.2 * 2 * e(coarse, fine) / n
    want_fine = 0.1 * 2 * e(fine, data) * sd / cnt - 0.2 * 2 * e(coarse, fine) / n
    want_aug = -0.1 * 2 * e(coarse, aug) / n + 0.5 * 2 * e(aug, data) * sd / cnt
    for got, want in ((grads[1], want_coarse), (grads[0], want_fine), (grads[3], want_aug)):
        assert float((got.double() - want).abs().max()) <= 2e-6 * float(want.abs().max())
    again = ops.loss_backward(terms, 4, scales, up, [True] * 4, [False, True, True, False])
    assert all(torch.equal(x, y) for x, y in zip(grads, again[0]))


def test_one_sided_terms_do_not_notice_a_two_sided_neighbour(monkeypatch):
    """The table LossComputer builds for the ``losses_full`` fixture, evaluated alone and with one two-sided term appended
    (depth_coarse against depth_fine, in a group of its own): term values, per-loss sums and d_pred of the original terms are
    bit-identical for every pred the added term does not touch."""
    g = util.load('losses_full.npz')
    configs, inp, out = util.loss_case(g, DEV)
    inp['common_data'] = {k: (v[None] if isinstance(v, torch.Tensor) else v) for k, v in inp['common_data'].items()}
    seen = {}
    forward = ops.loss_forward
    monkeypatch.setattr(ops, 'loss_forward', lambda terms, groups: (seen.update(terms=list(terms), groups=groups), forward(terms, groups))[1])
    LossComputer(configs).compute_losses(inp, out)
    monkeypatch.undo()
    terms, groups = seen['terms'], seen['groups']
    count = len(terms)
    assert (count, groups) == (11, 9)
    coarse = next(t.pred for t in terms if t.pred.data_ptr() == out['depth_coarse'].data_ptr())
    fine = next(t.pred for t in terms if t.pred.data_ptr() == out['depth_fine'].data_ptr())
    extended = terms + [ops.LossTermSpec(coarse, fine, None, None, groups, 0.1, two_sided=True)]

    def run(table, num_groups, with_target):
        values, scales = ops.loss_forward(table, num_groups)
        up = torch.zeros(len(table) + num_groups + 1, device=DEV)
        up[-1] = 1.0
        wanted_target = [t.two_sided for t in table] if with_target else None
        result = ops.loss_backward(table, num_groups, scales, up, [True] * len(table), wanted_target)
        return values, scales, (result[0] if with_target else result)

    v0, s0, g0 = run(terms, groups, False)
    v1, s1, g1 = run(extended, groups + 1, True)
    assert torch.equal(v0[:count], v1[:count]) and torch.equal(s0, s1[:count])
    assert torch.equal(v0[count:count + groups], v1[count + 1:count + 1 + groups])
    touched = {coarse.data_ptr(), fine.data_ptr()}
    untouched = [i for i, t in enumerate(terms) if t.pred.data_ptr() not in touched]
    assert len(untouched) >= 5 and len(untouched) < count
    for i in untouched:
        assert torch.equal(g0[i], g1[i]), i
    # and with the extra term at weight 0 the touched buffers agree too (+ 0 * x)
    extended[-1] = ops.LossTermSpec(coarse, fine, None, None, groups, 0.0, two_sided=True)
    _, _, g2 = run(extended, groups + 1, True)
    assert all(torch.equal(g0[i], g2[i]) for i in range(count))


def test_two_runs_are_bit_identical():
    results = []
    for _ in range(2):
        configs, inp, out = case_inputs('dense_fine')
        losses = LossComputer(configs).compute_losses(inp, out)
        losses['TotalLoss'].backward()
        results.append(([losses['TotalLoss'].detach()] + [losses[c['name']]['loss_value'].detach() for c in configs['losses']],
                        {k: v.grad for k, v in out.items()}))
    assert all(torch.equal(a, b) for a, b in zip(results[0][0], results[1][0]))
    for k in results[0][1]:
        assert torch.equal(results[0][1][k], results[1][1][k]), k


def test_single_pass_iteration_matches_sub_batched_with_the_new_losses():
    """tests/test_gpu_optim.py::test_single_pass_iteration_matches_sub_batched with the 01 consistency losses and
    DenseDepthMSE01 in the list, and its bounds: the sub-batch slicing cuts the dense-depth columns like the others."""
    from simplenerf_amd import harness, optim as snerf_optim
    from simplenerf_amd.models.ModelFactory import get_model

    def run(single_pass):
        cfg = synth.with_overrides(synth.training_configs('fp32', num_rays=512, num_sparse=512), perturb=False, raw_noise_std=0.0)
        cfg['sub_batch_size'] = 512
        cfg['losses'] = synth.loss_configs01(iter_weighted=False, dense=True)
        cfg['data_loader']['dense_depth'] = {}
        model = get_model(cfg, None)
        shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
        model.load_state_dict({k: torch.from_numpy(v) for k, v in synth.synth_state_dict(shapes, 7, 200.0, 8.0).items()})
        model = model.to(DEV).train()
        batch = BatchAssembler(cfg, synth.training_scene(0, 3, 96, 128, sparse_fraction=0.05, dense_depth=True), DEV).get_next_batch(0)
        assert tuple(batch['dense_depth_values'].shape) == (1024, 1) and (batch['dense_depth_values'][512:] == -1).all()
        opt = snerf_optim.Adam(list(model.parameters()), lr=0.0)
        totals = harness.train_one_iter(model, LossComputer(cfg), opt, batch, cfg['sub_batch_size'], single_pass=single_pass)
        return {k: float(v) for k, v in totals.items()}, {n: p.grad.clone() for n, p in model.named_parameters()}

    ref_loss, ref_grads = run(False)
    got_loss, got_grads = run(True)
    assert ref_loss['DenseDepthMSE01'] > 0 and ref_loss['CoarseFineConsistencyLoss01'] > 0
    for k, v in ref_loss.items():
        print(f'single pass {k}: {got_loss[k]!r} sub-batched {v!r}')
        assert abs(got_loss[k] - v) <= 1e-5 * max(abs(v), 1e-6), (k, got_loss[k], v)
    for k, g in ref_grads.items():
        err = float((got_grads[k] - g).abs().max() / max(float(g.abs().max()), 1e-30))
        assert err < 1e-4, (k, err)


# ---------------------------------------------------------------------------------------------------- batch keys
def dense_scene(g, d, mode):
    from tests.test_gpu_batch import golden_scene
    scene = golden_scene(g)
    scene.update(dense_depths=d[f'{mode}_dense_depths'], dense_depth_weights=d['dense_depth_weights'])
    if mode == 'ndc':
        scene['dense_depths_ndc'] = d['ndc_dense_depths_ndc']
    return scene


def loader(mode, **extra):
    return {'data_loader': {'ndc': mode == 'ndc', 'num_rays': 96, 'sparse_depth': {'num_rays': 32}, 'dense_depth': {}, **extra},
            'device': [0]}


DENSE_KEYS = ('dense_depth_values', 'dense_depth_weights', 'dense_depth_values_ndc')


@pytest.mark.parametrize('mode', ['ndc', 'world'])
def test_dense_depth_batch_keys_reproduce_the_reference_bit_for_bit(mode):
    g, d = util.load('batch_assembly.npz'), util.load('batch_dense_depth.npz')
    asm = BatchAssembler(loader(mode), dense_scene(g, d, mode), DEV)
    halves = [BatchAssembler(loader(mode), dense_scene(g, d, mode), DEV, rank=r, world_size=2) for r in range(2)]
    for b in range(2):
        idx = torch.from_numpy(d[f'{mode}_batch{b}_indices'])
        batch = asm.get_next_batch(b, indices=idx[:96], indices_sparse=idx[96:])
        for k in DENSE_KEYS:
            if mode == 'world' and k.endswith('_ndc'):
                assert k not in batch
                continue
            got, ref = batch[k].cpu().numpy(), d[f'{mode}_batch{b}_{k}']
            assert got.dtype == ref.dtype and got.shape == ref.shape == (128, 1), k
            assert numpy.array_equal(got, ref), (b, k)
            assert (got[96:] == -1).all() and (got[:96] != -1).any()
        # a 2-rank shard of the batch, reassembled: a rank's rows are rows of the single-process batch
        parts = []
        for r, h in enumerate(halves):
            lo, count, _ = h._shard(0, 96)
            lo_sd, count_sd, _ = h._shard(0, 32)
            parts.append(h.get_next_batch(b, indices=idx[lo:lo + count], indices_sparse=idx[96 + lo_sd:96 + lo_sd + count_sd]))
            assert parts[-1]['rays_o'].shape[0] == 64
        for k in DENSE_KEYS:
            if k in batch:
                both = torch.cat([p[k][:48] for p in parts] + [p[k][48:] for p in parts])
                assert torch.equal(both, batch[k]), k
    without = BatchAssembler({'data_loader': {'ndc': mode == 'ndc', 'num_rays': 96}, 'device': [0]}, dense_scene(g, d, mode), DEV)
    assert not any(k in without.get_next_batch(0) for k in DENSE_KEYS)         # the keys are there only with the switch


def test_dense_depth_keys_follow_the_device_index_stream_and_its_shards():
    """With the assembler's own index stream (no replayed order): the dense columns are the tables at ``indices`` on the pixel
    rows, -1 on the others and on out-of-range indices; two ranks' rows tile the single-process batch; a full image gathers
    every row."""
    scene = synth.training_scene(0, 3, 48, 64, sparse_fraction=0.05, dense_depth=True)
    cfg = synth.training_configs('fp32', num_rays=500, num_sparse=32)
    cfg['data_loader']['dense_depth'] = {}
    one = BatchAssembler(cfg, scene, DEV)
    halves = [BatchAssembler(cfg, scene, DEV, rank=r, world_size=2) for r in range(2)]
    tables = {'dense_depth_values': scene['dense_depths'], 'dense_depth_weights': scene['dense_depth_weights'],
              'dense_depth_values_ndc': scene['dense_depths_ndc']}
    for it in range(3):
        batch = one.get_next_batch(it)
        m = batch['indices_mask_nerf']
        parts = [h.get_next_batch(it) for h in halves]
        idx = batch['indices'].cpu().numpy()
        for k, table in tables.items():
            got = batch[k].cpu().numpy()
            assert numpy.array_equal(got[:500, 0], table[idx[:500]]) and (got[500:] == -1).all(), k
            both = torch.cat([p[k][p['indices_mask_nerf']] for p in parts] + [p[k][~p['indices_mask_nerf']] for p in parts])
            assert torch.equal(both, torch.cat([batch[k][m], batch[k][~m]])), k
    odd = one.get_next_batch(0, indices=torch.tensor([5, -1, 3 * 48 * 64, 100]))
    assert odd['dense_depth_values'][:, 0].tolist() == [float(scene['dense_depths'][5]), -1.0, -1.0, float(scene['dense_depths'][100])]
    image = one.get_next_batch(7, image_num=1)
    assert numpy.array_equal(image['dense_depth_weights'].cpu().numpy()[:, 0], scene['dense_depth_weights'][48 * 64:2 * 48 * 64])
    del scene['dense_depths_ndc']
    with pytest.raises(RuntimeError, match='dense_depths_ndc'):
        BatchAssembler(cfg, scene, DEV)
    with pytest.raises(RuntimeError, match='pixel rays'):
        ops.gather_dense_depth(batch['indices'], 600, one.dense['dense_depths'], one.dense['dense_depth_weights'])


# ---------------------------------------------------------------------------------------------------- training
def _density_path(name):
    return 'pts_linears' in name or 'pts_output_linear' in name


def _train_inputs(dense):
    scene = synth.synth_scene(0)
    batch = synth.loss_batch(scene, 192, 64, 1)
    t = lambda a: torch.from_numpy(numpy.ascontiguousarray(a)).to(DEV)
    n = 256
    rays_d = t(batch['rays_d'])
    inp = {'iter_num': 0, 'rays_o': t(batch['rays_o']), 'rays_d': rays_d,
           'view_dirs': rays_d / rays_d.norm(dim=1, keepdim=True), 'near': torch.full((n, 1), 2.0, device=DEV),
           'far': torch.full((n, 1), 6.0, device=DEV), 'pixel_id': t(batch['pixel_id']), 'target_rgb': t(batch['target_rgb']),
           'indices_mask_nerf': t(batch['indices_mask_nerf']), 'indices_mask_sparse_depth': t(batch['indices_mask_sparse_depth']),
           'sparse_depth_values': t(batch['sparse_depth_values']),
           'common_data': {'poses': t(scene['poses'])[None], 'images': t(scene['images'])[None],
                           'intrinsics': t(scene['intrinsics'])[None], 'resolution': scene['resolution']}}
    if dense:
        inp['dense_depth_values'] = t(synth.dense_depth_column(batch, synth.dense_depth_tables(scene, 0), scene))
    return inp


@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
@pytest.mark.parametrize('variant', ['consistency01', 'dense_coarse_only'])
def test_the_new_losses_train_the_renderer(precision, variant):
    """The synthetic scene of tests/test_gpu_losses.py::test_losses_train_the_renderer_end_to_end, the three 02 consistency
    losses replaced by their 01 forms (or DenseDepthMSE01 on a coarse-only model).  Back-propagating the depth terms ALONE:
    depth depends on density only, so the density-path parameters of the main AND of the augmented models receive finite,
    non-zero gradients and the colour-path parameters exact zeros.  Then twelve Adam steps on the batch (jitter and density
    noise off, so that the objective is one function): the total loss ends below its first value."""
    from simplenerf_amd import optim as snerf_optim
    from simplenerf_amd.models.ModelFactory import get_model
    dense = variant == 'dense_coarse_only'
    configs = synth.with_overrides(synth.make_configs('config3'), perturb=False, raw_noise_std=0.0)
    configs['model']['hip_precision'] = precision
    configs['data_loader']['ndc'] = False
    configs['data_loader']['sparse_depth'] = {}
    if dense:
        del configs['model']['fine_mlp']
        configs['data_loader']['dense_depth'] = {}
        configs['losses'] = synth.loss_configs()[:6] + [{'name': 'DenseDepthMSE01', 'weight': 0.1}]
        depth_losses = ['DenseDepthMSE01']
        reached = ['coarse_model']
    else:
        configs['losses'] = synth.loss_configs01(iter_weighted=False)
        depth_losses = ['PointsAugmentationDepthLoss01', 'ViewsAugmentationDepthLoss01', 'CoarseFineConsistencyLoss01']
        reached = ['coarse_model', 'fine_model', 'pts_aug_coarse_model', 'views_aug_coarse_model']
    torch.manual_seed(0)
    model = get_model(configs, None).to(DEV).train()
    computer = LossComputer(configs)
    inp = _train_inputs(dense)

    def losses_of():
        piece = dict(inp)
        piece['common_data'] = dict(inp['common_data'])
        return computer.compute_losses(piece, model(piece))

    losses = losses_of()
    sum(losses[name]['loss_value'] for name in depth_losses).backward()
    sigma_rows = {}
    for name, p in model.named_parameters():
        grad = torch.zeros_like(p) if p.grad is None else p.grad
        assert bool(torch.isfinite(grad).all()), name
        if not any(name.startswith(prefix) for prefix in reached):
            assert not grad.any(), name
        elif 'pts_output_linear' in name and p.shape[0] == 4:           # a view-independent head: row 0 is sigma, rows 1: colour
            assert not grad[1:].any(), name
            sigma_rows[name] = float(grad[0].abs().max() if grad.dim() == 2 else grad[0].abs())
        elif _density_path(name):
            sigma_rows[name] = float(grad.abs().max())
        else:
            assert not grad.any(), name                                  # feature_linear, views_linears, views_output_linear
    for prefix in reached:
        mine = {k: v for k, v in sigma_rows.items() if k.startswith(prefix)}
        assert mine and all(v > 0 for k, v in mine.items() if k.endswith('.weight')), (prefix, mine)
    opt = snerf_optim.Adam(list(model.parameters()), lr=5e-4)
    history = []
    for _ in range(12):
        opt.zero_grad(set_to_none=True)
        losses = losses_of()
        losses['TotalLoss'].backward()
        opt.step()
        history.append(float(losses['TotalLoss'].detach()))
    print(f'{variant} {precision}: TotalLoss {history[0]:.6f} -> {history[-1]:.6f}')
    assert numpy.isfinite(history).all() and history[-1] < history[0], history


@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
def test_graphed_whole_iteration_with_dense_depth_across_a_weight_change(precision):
    """harness.GraphedIteration with ``dense_depth`` on and the 01 losses in the list: the dense-depth gather reads the index
    buffer the graph's own permutation kernel fills, so it is part of the one graph.  Iterations 9997..10002 step the
    consistency weights from 0 to 0.1 at 10000 (a re-capture): loss values and every parameter bit-identical to the eager
    trainer iteration, as tests/test_gpu_optim.py demands of the shipped losses."""
    from simplenerf_amd import harness, optim
    from simplenerf_amd.lr_decayers.LearningRateDecayerFactory import get_lr_decayer
    from simplenerf_amd.models.ModelFactory import get_model
    cfg = synth.training_configs(precision, num_rays=192, num_sparse=64)
    cfg['sub_batch_size'] = 128
    cfg['losses'] = synth.loss_configs01(iter_weighted=True, dense=True)
    cfg['data_loader']['dense_depth'] = {}
    scene = synth.training_scene(0, 3, 48, 64, sparse_fraction=0.3, dense_depth=True)       # no short batch inside the run
    models = []
    for _ in range(2):
        m = get_model(cfg, None)
        shapes = {k: tuple(v.shape) for k, v in m.state_dict().items()}
        m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.synth_state_dict(shapes, 9, 200.0, 8.0).items()})
        models.append(m.to(DEV).train())
    eager, graphed = models
    batch_e, batch_g = BatchAssembler(cfg, scene, DEV), BatchAssembler(cfg, scene, DEV)
    losses = LossComputer(cfg)
    decayer = get_lr_decayer(cfg)
    opt_e, opt_g = optim.Adam(list(eager.parameters()), lr=5e-4), optim.Adam(list(graphed.parameters()), lr=5e-4)
    step = harness.GraphedIteration(graphed, losses, opt_g, batch_g, decayer, sub_batch_size=128, slots=4)
    captures, totals_seen = 0, []
    for it in range(9997, 10003):
        for group in opt_e.param_groups:
            group['lr'] = decayer.get_updated_learning_rate(it)
        batch = batch_e.get_next_batch(it)
        assert batch['rays_o'].shape[0] == 256 and 'dense_depth_values' in batch
        ref = harness.train_one_iter(eager, losses, opt_e, batch, 128)
        before = step.graph
        got = step(it)
        captures += step.graph is not before
        assert not step.last_was_short
        assert float(got['TotalLoss']) == float(ref['TotalLoss']), it
        assert sorted(got) == sorted(ref) and all(float(got[k]) == float(ref[k]) for k in ref), it
        totals_seen.append(float(got['DenseDepthMSE01']))
    assert captures == 2 and all(v > 0 for v in totals_seen)
    for (name, a), b in zip(eager.named_parameters(), graphed.parameters()):
        assert torch.equal(a, b), name
