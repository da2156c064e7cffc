#!/usr/bin/env python3
"""Time the density field's gradient on the device, launch by launch, beside what central differences would cost.  A record, not a
gate (needs the GPU).

    python tools/measure_field_gradient.py [--points 65536 1048576] [--repeats 5] [--out profiles/field_gradient.json]

The model is the seeded 8 x 256 / 128 coarse + fine NDC model of ``synth.make_configs('config2')`` (weights of
``synth.synth_state_dict(shapes, 31, 50.0, 2.0)``), its fine MLP asked at uniform random points of [-1, 1]^3, in blocks of 2^16
points (what ``model.query_gradient`` holds at a time), each figure the median over ``repeats`` rounds after one warm round of the
sum over the blocks:
  forward_train_event_ms   HIP events around the storing forward (``PackedMlp.forward_train``, S = 1, fp32)
  input_gradient_event_ms  HIP events around ``PackedMlp.input_gradient``: the clear, the backward chain and the new kernel
  chain_kernel_ms, encoding_kernel_ms, clear_kernel_ms
                           that call's three kernels apart, from the kernel records of ``torch.profiler`` over one more round (events
                           cannot be placed inside a library call); absent when the profiler reports no device activity
  normals_event_ms         HIP events around ``ops.field_normals`` with the NDC pull-back
  query_gradient_event_ms  HIP events around the whole ``model.query_gradient``
  six_queries_event_ms     HIP events around six ``model.query`` calls on the same points: the forwards of central differences"""
import argparse
import json
import os
import statistics
import sys

import numpy
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from simplenerf_amd import geometry, ops, synth  # noqa: E402
from simplenerf_amd.models.ModelFactory import get_model  # noqa: E402

DEV = 'cuda:0'
BLOCK = 1 << 16
KERNELS = {'chain_kernel_ms': 'mlp_backward_chain_kernel', 'encoding_kernel_ms': 'mlp_input_grad_kernel', 'clear_kernel_ms': 'clear_words_kernel'}


def spread(samples):
    return {'median': statistics.median(samples), 'min': min(samples), 'max': max(samples)}


def event_ms(fn):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    out = fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop), out


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--points', type=int, nargs='+', default=(1 << 16, 1 << 20))
    parser.add_argument('--repeats', type=int, default=5)
    parser.add_argument('--out', default=None)
    args = parser.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('measure_field_gradient: no GPU; nothing is measured without one')

    cfg = synth.make_configs('config2')
    model = get_model(cfg, None)
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    model.load_state_dict({k: torch.from_numpy(v) for k, v in synth.synth_state_dict(shapes, 31, 50.0, 2.0).items()})
    model = model.to(DEV).eval()
    params = model.fine_model.abi_params()
    packed = ops.PackedMlp(cfg['model']['fine_mlp'], DEV)
    packed.pack(params, ops.PRECISION_FP32, True)
    ndc = geometry.ndc_parameters(synth.camera('fern', 0))
    record = {'what': 'the density field\'s gradient (model.query_gradient) launch by launch, beside six model.query calls',
              'device': torch.cuda.get_device_name(0), 'model': 'config2, 8 x 256 / 128 fine MLP, seeded, fp32', 'point_block': BLOCK,
              'repeats': args.repeats, 'runs': []}
    zeros = torch.zeros((BLOCK, 3), device=DEV)
    depths = torch.zeros((BLOCK, 1), device=DEV)
    down = torch.tensor([0.0, 0.0, -1.0], device=DEV).expand(BLOCK, 3).contiguous()
    ones = torch.ones((BLOCK,), device=DEV)
    work = torch.empty(packed.input_gradient_workspace_floats(BLOCK), device=DEV)
    for n in args.points:
        rng = numpy.random.RandomState(n % 1000)
        points = torch.from_numpy(rng.uniform(-1, 1, (n, 3)).astype(numpy.float32)).to(DEV)
        scene = points.clone()
        scene[:, 2] = -ndc[2] - 0.5 - scene[:, 2].abs()              # scene-frame points in front of the near plane, for the pull-back
        series = {key: [] for key in ('forward_train', 'input_gradient', 'normals', 'query_gradient', 'six_queries')}

        def one_round(sample):
            grad = torch.empty((n, 3), device=DEV)
            for first in range(0, n, BLOCK):
                rows = min(BLOCK, n - first)
                ms, (sigma, _, saved) = event_ms(lambda: packed.forward_train(points[first:first + rows], zeros[:rows], down[:rows],
                                                                              depths[:rows], None, ops.PRECISION_FP32))
                sample['forward_train'] += ms
                ms, grad[first:first + rows] = event_ms(lambda: packed.input_gradient(params, saved, sigma, ones[:rows], work))
                sample['input_gradient'] += ms
            return grad

        for repeat in range(args.repeats + 1):                       # (round 0 warms every route)
            sample = dict.fromkeys(series, 0.0)
            grad = one_round(sample)
            sample['normals'], _ = event_ms(lambda: ops.field_normals(scene, grad, ndc))
            sample['query_gradient'], whole = event_ms(lambda: model.query_gradient(points, point_block=BLOCK))
            assert torch.equal(whole['grad'], grad)
            sample['six_queries'], _ = event_ms(lambda: [model.query(points, point_block=BLOCK) for _ in range(6)])
            if repeat:
                for key in series:
                    series[key].append(sample[key])
            print(f'{n} points round {repeat}: ' + ', '.join(f'{key} {sample[key]:.3f} ms' for key in series), file=sys.stderr, flush=True)
        run = {'points': n, 'closed_share': float((whole['sigma'] == 0).float().mean())}
        run.update({f'{key}_event_ms': spread(samples) for key, samples in series.items()})
        run['gradient_points_per_s'] = n / (statistics.median(series['query_gradient']) * 1e-3)
        try:                                                         # the library call's kernels apart
            from torch.profiler import ProfilerActivity, profile
            with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
                one_round(dict.fromkeys(series, 0.0))
                torch.cuda.synchronize()
            device_us = lambda e: getattr(e, 'device_time', None) or getattr(e, 'cuda_time', 0) or 0      # (the attribute's name by torch version)
            for key, name in KERNELS.items():
                found = [e for e in prof.events() if name in e.name and device_us(e) > 0]
                if found:
                    run[key] = sum(device_us(e) for e in found) * 1e-3
                    run[key.replace('_ms', '_launches')] = len(found)
        except Exception as error:                                   # a record without the split is still a record
            run['profiler_error'] = repr(error)
        record['runs'].append(run)
    line = json.dumps(record)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
