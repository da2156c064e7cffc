"""The model under ``torch.nn.DataParallel`` with SEVERAL device ids, as every shipped demo configures it (``'device': [0, 1]``;
src/Trainer01.py:514, src/Tester01.py:42).  The test box has one MI355X, so the core cases repeat the id: ``device_ids=[0, 0]``
takes the whole multi-device path on one card -- replicate (broadcast copies of the weights, held by replicas that have no
``parameters()``), scatter of the batch, two replicas in ``parallel_apply``'s threads enqueuing on ONE stream, gather, and
``Broadcast``'s backward summing the replicas' returned gradients onto the parameters.  With two or more GPUs the training and
frame cases run with ``[0, 1]`` as well.

Gates: forward outputs bit-equal to the unwrapped model (no arithmetic crosses rays); the trainer loop's losses bit-equal in its
first iteration and gradients within 2e-5 of each tensor's largest entry (two replicas' sums added in another order, the bound
of tests/test_gpu_dist.py); parameters after three Adam steps within the bound Adam itself puts on a step; one replica by hand
bit-equal (gradient routing alone); named errors for what a replica cannot do; and two host threads rendering on one stream
bit-equal to the same calls made one after another."""
import copy
import threading

import pytest
import torch
from torch.nn.parallel import gather, parallel_apply, replicate, scatter

from simplenerf_amd import harness, ops, synth
from simplenerf_amd.data_preprocessors.BatchAssembler01 import BatchAssembler
from simplenerf_amd.loss_functions.LossComputer01 import LossComputer
from simplenerf_amd.lr_decayers.LearningRateDecayerFactory import get_lr_decayer
from tests import util
from tests.test_gpu_dataparallel import _fresh_model, _trainer_iteration

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
DEVICE_IDS = [pytest.param([0, 0], id='0,0'),
              pytest.param([0, 1], id='0,1', marks=pytest.mark.skipif(torch.cuda.device_count() < 2, reason='needs two GPUs'))]


def _layered(cfg):
    """``cfg`` with 8 x 512 coarse and fine MLPs: a shape outside the fused kernels' set (the layered path, csrc/mlp_generic.hip)."""
    cfg = copy.deepcopy(cfg)
    for level in ('coarse', 'fine'):
        cfg['model'][f'{level}_mlp'] = synth.mlp_config(cfg['model'][f'{level}_mlp']['num_samples'], width=512)
    return cfg


def _with_devices(cfg, device_ids):
    cfg = copy.deepcopy(cfg)
    cfg['device'] = list(device_ids)
    return cfg


def _assert_same_outputs(got, expected, tag):
    assert list(got.keys()) == list(expected.keys()), tag
    for key in expected:
        assert got[key].device == expected[key].device and torch.equal(got[key], expected[key]), (tag, key)


# ------------------------------------------------------------------------------------------------ the reference's trainer loop
@pytest.mark.parametrize('device_ids', DEVICE_IDS)
@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
def test_trainer_loop_over_two_replicas(precision, device_ids):
    """BASELINE config 5 (2048 pixel + 2048 sparse rows, two sub-batches, the nine losses) driven by the reference's loop on
    ``DataParallel(model, device_ids)`` against the unwrapped model on the same batches.  Two runs: with lr = 0 every iteration's
    forward sees the same weights, so every iteration's losses are bit-equal and its gradients within 2e-5; with the real Adam
    and LR decayer the parameters after three steps stay within 3 x 2.02 x lr of each other -- a step of Adam moves a parameter
    by at most ~1.01 lr in the first three iterations (beta1 0.9, beta2 0.999), and a near-zero gradient whose sign rounding
    flips turns into that whole step."""
    cfg = synth.training_configs(precision, num_rays=2048, num_sparse=2048)
    cfg_w = _with_devices(cfg, device_ids)
    scene = synth.training_scene(sparse_points=2048 * 16)
    decayer = get_lr_decayer(cfg)
    for adam in (False, True):
        wrapped = torch.nn.DataParallel(_fresh_model(cfg_w), device_ids=device_ids).to(DEV).train()
        plain = _fresh_model(cfg).to(DEV).train()
        make = lambda m: torch.optim.Adam(list(m.parameters()), lr=0.0, betas=(cfg['optimizer']['beta1'], cfg['optimizer']['beta2']))
        opt_w, opt_p = make(wrapped), make(plain)
        batcher_w, batcher_p = BatchAssembler(cfg_w, scene, DEV), BatchAssembler(cfg, scene, DEV)
        losses_w, losses_p = LossComputer(cfg_w), LossComputer(cfg)
        lrs = []
        for step, it in enumerate((20000, 20001, 20002)):
            lr = decayer.get_updated_learning_rate(it) if adam else 0.0
            lrs.append(lr)
            for opt in (opt_w, opt_p):
                for group in opt.param_groups:
                    group['lr'] = lr
            batch_w, batch_p = batcher_w.get_next_batch(it), batcher_p.get_next_batch(it)
            assert batch_w['common_data']['poses'].shape[0] == 2 and batch_p['common_data']['poses'].shape[0] == 1
            totals_w = _trainer_iteration(wrapped, losses_w, opt_w, batch_w, cfg_w)
            totals_p = _trainer_iteration(plain, losses_p, opt_p, batch_p, cfg)
            assert set(totals_w) == set(totals_p) and float(totals_p['TotalLoss']) > 0
            if not adam or step == 0:
                for name in totals_p:
                    assert totals_w[name] == totals_p[name], (adam, it, name, totals_w[name], totals_p[name])
                for (name, pw), pp in zip(wrapped.module.named_parameters(), plain.parameters()):
                    assert pw.grad is not None and pp.grad is not None, name
                    scale = float(pp.grad.abs().max())
                    diff = float((pw.grad - pp.grad).abs().max())
                    assert scale > 0 and diff <= 2e-5 * scale, (adam, it, name, diff / scale)
        if adam:
            bound = 3 * 2.02 * max(lrs)
            worst = max(float((pw.detach() - pp.detach()).abs().max()) for pw, pp in zip(wrapped.module.parameters(), plain.parameters()))
            moved = max(float((pw.detach() - p0.to(DEV)).abs().max())
                        for pw, p0 in zip(wrapped.module.parameters(), _fresh_model(cfg).parameters()))
            util.observe(f'dataparallel_devices/{precision}/{device_ids}', f'parameters after 3 Adam steps: max |wrapped - unwrapped| '
                                                                           f'{worst:.2e} [{bound:.2e}], largest move {moved:.2e}')
            assert moved > 0 and worst <= bound, (worst, bound)


# ------------------------------------------------------------------------------------------------ forward outputs, bit for bit
@pytest.mark.parametrize('device_ids', DEVICE_IDS)
@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
@pytest.mark.parametrize('shape', ['fused', 'layered'])
def test_forward_outputs_are_bit_equal(shape, precision, device_ids):
    """The tester's call (a whole fern frame, no_grad, ``sec_views_vis=False``; the layered shape on a quarter-resolution frame)
    and a training forward of an assembled batch with ``retraw``: every output equal to the unwrapped model's."""
    base = synth.with_overrides(synth.make_configs('config2'), hip_precision=precision)
    cfg = _layered(base) if shape == 'layered' else base
    cfg_w = _with_devices(cfg, device_ids)
    wrapped = torch.nn.DataParallel(_fresh_model(cfg_w), device_ids=device_ids).to(DEV).eval()
    plain = _fresh_model(cfg).to(DEV).eval()
    cam = synth.camera('fern', 0, downscale=4 if shape == 'layered' else 1)
    frame = harness.frame_batch(cam, True, DEV)
    assert frame['rays_o'].shape[0] == cam['resolution'][0] * cam['resolution'][1]
    with torch.no_grad():
        _assert_same_outputs(wrapped(frame, sec_views_vis=False), plain(frame, sec_views_vis=False), 'frame')
        _assert_same_outputs(wrapped(frame, retraw=True), plain(frame, retraw=True), 'frame/retraw')

    tcfg = synth.training_configs(precision, num_rays=1024, num_sparse=512)
    tcfg = _layered(tcfg) if shape == 'layered' else tcfg
    tcfg_w = _with_devices(tcfg, device_ids)
    scene = synth.training_scene(sparse_points=512 * 16)
    wrapped = torch.nn.DataParallel(_fresh_model(tcfg_w), device_ids=device_ids).to(DEV).train()
    plain = _fresh_model(tcfg).to(DEV).train()
    batch_w, batch_p = BatchAssembler(tcfg_w, scene, DEV).get_next_batch(7), BatchAssembler(tcfg, scene, DEV).get_next_batch(7)
    out_w, out_p = wrapped(batch_w, retraw=True), plain(batch_p, retraw=True)
    assert out_w['rgb_fine'].requires_grad and 'raw_sigma_fine' in out_w and 'points_augmentation_rgb_coarse' in out_w
    _assert_same_outputs({k: v.detach() for k, v in out_w.items()}, {k: v.detach() for k, v in out_p.items()}, 'train')


# ------------------------------------------------------------------------------------------------ gradient routing alone
@pytest.mark.parametrize('binding', ['torch_ext', 'ctypes'])
def test_one_replica_by_hand_gives_the_same_gradients(binding):
    """``replicate(model, [0])`` + ``parallel_apply`` + ``gather``: the replica returns its gradients through autograd (its weights
    are broadcast copies, not leaves) and ``Broadcast``'s backward hands them to the parameters -- bit-equal to the unwrapped
    model's direct writes, since one replica sums nothing."""
    cfg = synth.training_configs('fp32', num_rays=1024, num_sparse=512)
    cfg['model']['hip_host_binding'] = binding
    scene = synth.training_scene(sparse_points=512 * 16)
    model, plain = _fresh_model(cfg).to(DEV).train(), _fresh_model(cfg).to(DEV).train()
    batch = BatchAssembler(cfg, scene, DEV).get_next_batch(3)
    replicas = replicate(model, [0])
    assert len(replicas) == 1 and replicas[0]._is_replica and not list(replicas[0].parameters())
    inputs = scatter((batch,), [0])
    out = gather(parallel_apply(replicas, inputs, None, [0]), 0)
    util.grad_loss(out).backward()
    util.grad_loss(plain(batch)).backward()
    for (name, p), q in zip(model.named_parameters(), plain.parameters()):
        assert p.grad is not None and torch.equal(p.grad, q.grad), name
    # the replica packed into a cache of its own: the model's holds nothing it did not pack itself
    assert not model._packed and replicas[0]._packed


# ------------------------------------------------------------------------------------------------ batch assembly
def test_common_data_has_one_copy_per_device():
    cfg = synth.training_configs('fp32', num_rays=256, num_sparse=128)
    scene = synth.training_scene(sparse_points=4096)
    one = BatchAssembler(cfg, scene, DEV).get_next_batch(0)
    batcher = BatchAssembler(_with_devices(cfg, [0, 0]), scene, DEV)
    two = batcher.get_next_batch(0)
    for key in ('poses', 'intrinsics', 'images'):
        single, pair = one['common_data'][key], two['common_data'][key]
        assert single.shape[0] == 1 and single.is_contiguous() and pair.shape == (2,) + single.shape[1:]
        assert pair.stride(0) == 0 and pair.data_ptr() == getattr(batcher, key).data_ptr()      # an expanded view, no copy
        assert torch.equal(pair[1], single[0])
    assert one['common_data']['resolution'] == two['common_data']['resolution']
    for key in one:
        if torch.is_tensor(one[key]):
            assert torch.equal(one[key], two[key]), key
    shares = scatter((two,), [0, 0])
    assert len(shares) == 2
    for (share,) in shares:
        assert share['rays_o'].shape[0] == 192 and share['global_rows'].shape == (192,)
        assert share['common_data']['poses'].shape == (1,) + one['common_data']['poses'].shape[1:]
        assert share['iter_num'] == 0 and share['common_data']['resolution'] == one['common_data']['resolution']
    # with [0] the scatter hands the whole batch to the one replica, as before
    assert len(scatter((one,), [0])) == 1


# ------------------------------------------------------------------------------------------------ named errors
def _training_pair(precision='fp32'):
    cfg = _with_devices(synth.make_configs('config3'), [0, 0])
    cfg['model']['hip_precision'] = precision
    return torch.nn.DataParallel(_fresh_model(cfg), device_ids=[0, 0]).to(DEV).train()


def test_a_replica_needs_global_rows_and_iter_num():
    wrapped = _training_pair()
    cam = synth.camera('fern', 0)
    batch = harness.frame_batch(cam, True, DEV, 300000, 512)
    batch['iter_num'] = 5
    with pytest.raises(RuntimeError, match=r"input_batch\['global_rows'\] is required"):
        wrapped(batch)
    batch['global_rows'] = torch.arange(512, dtype=torch.int64, device=DEV)
    del batch['iter_num']
    with pytest.raises(RuntimeError, match=r"input_batch\['iter_num'\] is required"):
        wrapped(batch)
    batch['iter_num'] = 5
    out = wrapped(batch)
    assert out['rgb_fine'].shape == (512, 3)
    # no draws, no keys needed: eval mode
    wrapped.eval()
    del batch['iter_num'], batch['global_rows']
    with torch.no_grad():
        assert wrapped(batch)['rgb_fine'].shape == (512, 3)


def test_set_random_draws_refuses_a_replicated_call():
    wrapped = _training_pair()
    cam = synth.camera('fern', 0)
    batch = harness.frame_batch(cam, True, DEV, 300000, 256)
    batch.update(iter_num=1, global_rows=torch.arange(256, dtype=torch.int64, device=DEV))
    wrapped.module.set_random_draws({'t_rand': torch.rand(256, 64, device=DEV)})
    with pytest.raises(RuntimeError, match='set_random_draws'):
        wrapped(batch)


def test_fp16_range_error_keeps_its_type_through_the_replicas():
    """The reference's wrapper re-raises a replica's exception by constructing its type from the message
    (``ExceptionWrapper.reraise``): an out-of-range fp16 call still surfaces as ``Fp16RangeError``.  The range flag is one per
    device, so on ``[0, 0]`` the other replica of the SAME call may be the one that reports it -- by the next call at the latest."""
    cfg = _with_devices(synth.with_overrides(synth.make_configs('config2'), hip_precision='f16'), [0, 0])
    wrapped = torch.nn.DataParallel(_fresh_model(cfg), device_ids=[0, 0]).to(DEV).eval()
    batch = harness.frame_batch(synth.camera('fern', 0), True, DEV, 200000, 64)
    ops.range_status(clear=True)
    with torch.no_grad():
        assert torch.isfinite(wrapped(batch)['rgb_fine']).all()
        torch.cuda.synchronize()
        assert ops.range_status() == 0
        wrapped.module.coarse_model.pts_linears[2].bias[17] = 1.0e5
        with pytest.raises(ops.Fp16RangeError, match='fp16 range'):
            wrapped(batch)
            torch.cuda.synchronize()
            wrapped(batch)
    torch.cuda.synchronize()
    ops.range_status(clear=True)


# ------------------------------------------------------------------------------------------------ the library from two threads
def _thread_case(kind):
    if kind == 'layered':        # the inference scratch block of the layered path (one per device and stream), 13 passes a call
        cfg = _layered(synth.make_configs('config2'))
        models = [_fresh_model(cfg, seed).to(DEV).eval() for seed in (7, 8)]
        cam = synth.camera('fern', 0)
        batches = [harness.frame_batch(cam, True, DEV, 200000 + 3000 * i, 2048) for i in range(2)]
        return models, batches, False
    # four levels below the side-by-side limit (512 rays x 64 coarse samples): side streams, fork and join events
    cfg = synth.make_configs('config3')
    models = [_fresh_model(cfg, seed).to(DEV).train() for seed in (7, 8)]
    cam = synth.camera('fern', 0)
    batches = []
    for i in range(2):
        batch = harness.frame_batch(cam, True, DEV, 250000 + 1000 * i, 512)
        batch.update(iter_num=4 + i, global_rows=torch.arange(512, dtype=torch.int64, device=DEV) + 512 * i)
        batches.append(batch)
    return models, batches, True


def _run(model, batch, train):
    if not train:
        with torch.no_grad():
            return {k: v.clone() for k, v in model(batch, retraw=True).items()}
    for p in model.parameters():
        p.grad = None
    out = model(batch)
    util.grad_loss(out).backward()
    result = {k: v.detach().clone() for k, v in out.items()}
    result.update({'grad.' + k: p.grad.clone() for k, p in model.named_parameters()})
    return result


@pytest.mark.parametrize('kind', ['layered', 'side_by_side'])
def test_two_threads_on_one_stream(kind):
    """Two Python threads, each rendering its own model 20 times on device 0 and the SAME stream (the device's current one): every
    result bit-equal to the same call made alone."""
    models, batches, train = _thread_case(kind)
    alone = [_run(m, b, train) for m, b in zip(models, batches)]
    torch.cuda.synchronize()
    results, errors = [[], []], []
    start = threading.Barrier(2)

    def work(i):
        try:
            assert torch.cuda.current_stream(0) == torch.cuda.default_stream(0)
            start.wait()
            for _ in range(20):
                results[i].append(_run(models[i], batches[i], train))
        except BaseException as error:       # (reported below, in the test's thread)
            errors.append(error)

    threads = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    torch.cuda.synchronize()
    assert not errors, errors
    for i in range(2):
        assert len(results[i]) == 20
        for rep, got in enumerate(results[i]):
            assert got.keys() == alone[i].keys()
            for key in alone[i]:
                assert torch.equal(got[key], alone[i][key]), (i, rep, key)


def test_graphed_steps_refuse_a_multi_device_wrapper():
    wrapped = _training_pair()
    with pytest.raises(NotImplementedError, match='GraphedTrainStep: a DataParallel wrapper over several devices'):
        harness.GraphedTrainStep(wrapped, None, {})
    with pytest.raises(NotImplementedError, match='GraphedIteration: a DataParallel wrapper over several devices'):
        harness.GraphedIteration(wrapped, None, None, None)
