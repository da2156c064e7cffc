#!/usr/bin/env python3
"""Time the static-camera view sweep against the loop it replaces.  A record, not a gate (needs the GPU).

    python tools/measure_view_sweep.py [--views 16] [--repeats 3] [--resolution 756 1008] [--precision fp32] [--out FILE]
                                                                                                            -> one JSON line

One fern frame (756 x 1008), 64 + 128 samples, 8 x 256 coarse + fine, V view cameras scattered around the frame's own, at
``--precision`` (fp32, f16, bf16, f16s8 or bf16s8: a mode with a one-trunk-pass route):
  sweep_ms     ``harness.predict_view_sweep`` on its fast route (default ray block), HIP events around the whole call
  parts_ms     the same block loop with events around its three parts, summed over the blocks: the keep-activations render,
               ``ops.view_sweep`` (``ops.view_sweep_half`` in the 16-bit modes), the display conversions (the parts add up to less than the sweep: ray generation, the copies into
               the frame buffers and the copy of the images to the host are outside them)
  loop_ms      V ordinary renders of the frame at the same precision (``harness.predict_frame(view_camera=...)``): what the
               fallback route, and the code before the mode's sweep existed, needs
  ratio        loop_ms / sweep_ms
Each figure is the median of ``repeats`` runs after one warm run; the spread (min, max) is recorded beside it."""
import argparse
import json
import os
import statistics
import sys

import numpy
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from simplenerf_amd import harness, ops, synth  # noqa: E402
from simplenerf_amd.models.ModelFactory import get_model  # noqa: E402

DEV = 'cuda:0'


def timed(fn, repeats):
    """Median / min / max of ``repeats`` runs of ``fn`` in ms (HIP events on the current stream), after one warm run."""
    fn()
    torch.cuda.synchronize()
    samples = []
    for _ in range(repeats):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        fn()
        stop.record()
        stop.synchronize()
        samples.append(start.elapsed_time(stop))
    return {'median': statistics.median(samples), 'min': min(samples), 'max': max(samples)}


def sweep_parts(model, configs, camera, view_cameras, block):
    """The block loop of predict_view_sweep's fast route with events around its parts -> {part: ms summed over the blocks}."""
    mcfg = configs['model']
    h, w = camera['resolution']
    packed = [model._packed_mlp('coarse_model', True), None, None, model._packed_mlp('fine_model', True), None, None]
    params = model.fine_model.abi_params()
    marks = []
    for first in range(0, h * w, block):
        rays = min(block, h * w - first)
        batch = harness.frame_batch(camera, True, DEV, first, rays)
        dirs = torch.stack([harness.view_directions(camera, c, DEV, first, rays) for c in view_cameras])
        events = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        events[0].record()
        kept = ops.render_keep_activations(packed, batch, True, False, False, mcfg['coarse_mlp']['num_samples'], mcfg['fine_mlp']['num_samples'],
                                           precision=model.precision)
        events[1].record()
        if model.precision == ops.PRECISION_FP32:
            swept = ops.view_sweep(packed[3], params, kept['saved_acts'], kept['weights'], kept['acc'], dirs, False)
        else:
            swept = ops.view_sweep_half(packed[3], params, kept['saved_acts'], kept['weights'], kept['acc'], dirs, False, model.precision)
        events[2].record()
        for v in range(len(view_cameras)):
            ops.to_display(swept[v], None)
        for name in ('depth', 'depth_var', 'depth_ndc', 'depth_var_ndc'):
            ops.to_display(None, kept['outputs'][name], colour=False)
        events[3].record()
        marks.append(events)
    torch.cuda.synchronize()
    names = ('keep_activations_render', 'view_sweep', 'display')
    return {name: sum(e[i].elapsed_time(e[i + 1]) for e in marks) for i, name in enumerate(names)}


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--views', type=int, default=16)
    parser.add_argument('--repeats', type=int, default=3)
    parser.add_argument('--resolution', type=int, nargs=2, default=None)
    parser.add_argument('--precision', default='fp32', choices=['fp32', 'f16', 'bf16', 'f16s8', 'bf16s8'])
    parser.add_argument('--out', default=None)
    args = parser.parse_args()

    configs = synth.with_overrides(synth.make_configs('config2'), hip_precision=args.precision)
    model = get_model(configs, None)
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    model.load_state_dict({k: torch.from_numpy(v) for k, v in synth.synth_state_dict(shapes, 0, sigma_gain=60.0).items()})
    model = model.to(DEV).eval()
    assert harness.view_sweep_is_fast(model)
    camera = synth.camera('fern', 0, resolution=args.resolution)
    rng = numpy.random.RandomState(0)
    view_cameras = []
    for _ in range(args.views):
        c = dict(camera)
        c['pose'] = camera['pose'].copy()
        c['pose'][:3, 3] += (0.3 * rng.standard_normal(3)).astype(numpy.float32)
        view_cameras.append(c)
    block = harness._sweep_ray_block(model, args.views)

    sweep = timed(lambda: harness.predict_view_sweep(model, configs, camera, view_cameras, DEV), args.repeats)
    print(f'sweep {sweep}', file=sys.stderr, flush=True)
    loop = timed(lambda: [harness.predict_frame(model, configs, camera, DEV, view_camera=c) for c in view_cameras], args.repeats)
    print(f'loop {loop}', file=sys.stderr, flush=True)
    sweep_parts(model, configs, camera, view_cameras, block)
    parts = [sweep_parts(model, configs, camera, view_cameras, block) for _ in range(args.repeats)]
    record = {'what': 'static-camera view sweep against V ordinary renders of the frame', 'device': torch.cuda.get_device_name(0),
              'resolution': list(camera['resolution']), 'samples': [64, 128], 'mlp': f'8x256 / 1x128, {args.precision}', 'precision': args.precision, 'views': args.views,
              'repeats': args.repeats, 'ray_block': block, 'sweep_ms': sweep, 'loop_ms': loop,
              'parts_ms': {name: statistics.median(p[name] for p in parts) for name in parts[0]},
              'ratio': loop['median'] / sweep['median']}
    line = json.dumps(record)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
