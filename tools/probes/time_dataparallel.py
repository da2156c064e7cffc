"""The reference's training loop on ``torch.nn.DataParallel(model, device_ids)`` for the device lists given on the command line:
BASELINE config 5 (2048 pixel + 2048 sparse-depth rows, two sub-batches of 2048, the nine losses, Adam with the NeRF LR decay),
the loop of src/Trainer01.py:61-107 restated (zero_grad(set_to_none=True), every tensor of the batch sliced per sub-batch,
model -> compute_losses -> TotalLoss.backward(), loss values read with float(), one optimizer.step()).  One JSON line per case:
milliseconds per iteration (median of ``--rounds`` timed blocks of ``--steps`` iterations), then one line with the cost of the
re-pack a replica makes on every forward (a fresh packed buffer per MLP of the training forward, packed for training).

    python tools/probes/time_dataparallel.py [--device-ids "0;0,0;0,1"] [--precision fp32] [--steps 20] [--rounds 3]

``0`` is the reference's one-device wrapper (no replication: the unwrapped model's path), ``0,0`` two replicas on one GPU
(replicate, scatter, two threads, gather, reduce-add, re-packs: the wrapper's overhead), ``0,1`` two GPUs."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from simplenerf_amd import ops, synth  # noqa: E402
from simplenerf_amd.data_preprocessors.BatchAssembler01 import BatchAssembler  # noqa: E402
from simplenerf_amd.loss_functions.LossComputer01 import LossComputer  # noqa: E402
from simplenerf_amd.lr_decayers.LearningRateDecayerFactory import get_lr_decayer  # noqa: E402
from simplenerf_amd.models.ModelFactory import get_model  # noqa: E402


def fresh_model(cfg):
    model = get_model(cfg, None)
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    model.load_state_dict({k: torch.from_numpy(v) for k, v in synth.synth_state_dict(shapes, 7, 200.0, 8.0).items()})
    return model


def trainer_iteration(model, loss_computer, optimizer, batch, sub):
    optimizer.zero_grad(set_to_none=True)
    rows = batch['rays_o'].shape[0]
    total = 0.0
    for first in range(0, rows, sub):
        piece = {name: (value[first:first + sub] if torch.is_tensor(value) else
                        (value.copy() if name == 'common_data' else value)) for name, value in batch.items()}
        terms = loss_computer.compute_losses(piece, model(piece))
        terms['TotalLoss'].backward()
        total += sum(float(t['loss_value'] if isinstance(t, dict) else t) for t in terms.values())
    optimizer.step()
    return total


def time_case(device_ids, precision, steps, rounds, warmup):
    cfg = synth.training_configs(precision, num_rays=2048, num_sparse=2048)
    cfg['device'] = list(device_ids)
    dev = torch.device('cuda', device_ids[0])
    scene = synth.training_scene(sparse_points=2048 * 16)
    model = torch.nn.DataParallel(fresh_model(cfg), device_ids=device_ids).to(dev).train()
    optimizer = torch.optim.Adam(list(model.parameters()), lr=cfg['optimizer']['lr_initial'],
                                 betas=(cfg['optimizer']['beta1'], cfg['optimizer']['beta2']))
    decayer, losses, batcher = get_lr_decayer(cfg), LossComputer(cfg), BatchAssembler(cfg, scene, dev)
    it = 20000

    def step():
        nonlocal it
        for group in optimizer.param_groups:
            group['lr'] = decayer.get_updated_learning_rate(it)
        trainer_iteration(model, losses, optimizer, batcher.get_next_batch(it), cfg['sub_batch_size'])
        it += 1

    for _ in range(warmup):
        step()
    blocks = []
    for _ in range(rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            step()
        for d in set(device_ids):
            torch.cuda.synchronize(d)
        blocks.append((time.perf_counter() - t0) / steps * 1e3)
    return {'case': 'trainer_loop', 'device_ids': list(device_ids), 'precision': precision, 'rows': 4096, 'sub_batch_size': 2048,
            'steps': steps, 'rounds': rounds, 'ms_per_iteration': statistics.median(blocks), 'blocks_ms': blocks}


def time_repack(precision, steps):
    """What a replica adds per training forward: a new packed buffer per present MLP (allocation + zero fill) and its pack."""
    cfg = synth.training_configs(precision, num_rays=2048, num_sparse=2048)
    dev = torch.device('cuda', 0)
    model = fresh_model(cfg).to(dev).train()
    names = ['coarse_model', 'fine_model'] + [name for _, _, name in model._train_only]
    params = {name: getattr(model, name).abi_params() for name in names}

    def repack():
        for name in names:
            ops.PackedMlp(getattr(model, name).mlp_configs, dev).pack(params[name], model.precision, True)

    for _ in range(5):
        repack()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    start.record()
    for _ in range(steps):
        repack()
    stop.record()
    torch.cuda.synchronize()
    host = (time.perf_counter() - t0) / steps * 1e3
    return {'case': 'replica_repack', 'precision': precision, 'mlps': names, 'steps': steps, 'ms_per_forward_wall': host,
            'ms_per_forward_device': start.elapsed_time(stop) / steps,
            'per_iteration_note': 'a two-replica iteration of config 5 re-packs 2 sub-batches x 2 replicas = 4 times; '
                                  'the unwrapped model once (after the optimiser step)'}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--device-ids', default='0;0,0')
    ap.add_argument('--precision', default='fp32')
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=5)
    args = ap.parse_args()
    for case in args.device_ids.split(';'):
        ids = [int(d) for d in case.split(',')]
        if max(ids) >= torch.cuda.device_count():
            print(json.dumps({'case': 'trainer_loop', 'device_ids': ids, 'skipped': f'{torch.cuda.device_count()} GPU(s) visible'}), flush=True)
            continue
        print(json.dumps(time_case(ids, args.precision, args.steps, args.rounds, args.warmup)), flush=True)
    print(json.dumps(time_repack(args.precision, 50)), flush=True)


if __name__ == '__main__':
    main()
