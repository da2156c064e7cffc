#!/usr/bin/env python3
"""Time the normal maps of one full frame on the device, piece by piece, beside the plain render of the same frame.  A record, not a
gate (needs the GPU).

    python tools/measure_normals.py [--precisions fp32 bf16] [--repeats 3] [--resolution 756 1008] [--out profiles/normal_maps.json]

The model is the seeded 8 x 256 / 128 coarse + fine NDC model of ``synth.make_configs('config2')`` (64 + 128 samples; weights of
``synth.synth_state_dict(shapes, 31, 50.0, 2.0)``), the frame the fern camera's.  The seeded field is noise: what share of the
samples it selects says nothing about a trained model, and no trained model has been timed.  The pieces are those of
``harness.predict_normals``, in its blocks of ``harness.NORMALS_RAY_BLOCK`` rays, each figure the sum over the blocks by HIP events
(a pair of events per piece and block; the selection's and the gradient's include their read-backs and allocations), and per
precision the median, the smallest and the largest of ``repeats`` rounds after one warm round:
  render_event_ms          ``model(frame_batch(...), retraw=True)`` at the model's precision, the ray generation included
  select_event_ms          ``ops.select_ray_samples`` (count, scan, read-back of M, emit), min_weight 0
  gradient_event_ms        ``model.query_gradient`` at the selected points (always fp32), in blocks of 2^16 points
  composite_event_ms       ``ops.composite_normals`` with the NDC pull-back
  depth_normals_event_ms   ``geometry.depth_normals`` of the displayed depth map (its camera table built on the host each time)
  pictures_event_ms        both ``geometry.normals_to_u8`` calls
  predict_normals_ms       the whole ``harness.predict_normals``, wall clock to a synchronised device
  predict_frame_ms         ``harness.predict_frame`` of the same frame, wall clock (its five maps copied to the host)
``selected_fraction`` is the share of the frame's samples with weight > 0."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from simplenerf_amd import geometry, harness, ops, synth  # noqa: E402
from simplenerf_amd.models.ModelFactory import get_model  # noqa: E402

DEV = 'cuda:0'
PIECES = ('render', 'select', 'gradient', 'composite', 'depth_normals', 'pictures')


def spread(samples):
    return {'median': statistics.median(samples), 'min': min(samples), 'max': max(samples)}


def event_ms(fn):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    out = fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop), out


def wall_ms(fn):
    torch.cuda.synchronize()
    begin = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - begin) * 1e3, out


@torch.no_grad()
def one_frame(model, cfg, camera, sample):
    """harness.predict_normals, piece by piece; -> (normal, depth normal, selected samples, samples)."""
    device = torch.device(DEV)
    h, w = (int(v) for v in camera['resolution'])
    n, block = h * w, harness.NORMALS_RAY_BLOCK
    parameters = geometry.ndc_parameters(camera)
    normal = torch.empty((n, 3), device=device)
    rgb = torch.empty((n, 3), device=device)
    depth = torch.empty((n,), device=device)
    selected = samples = 0
    for start in range(0, n, block):
        count = min(block, n - start)
        ms, (batch, out) = event_ms(lambda: (lambda b: (b, model(b, retraw=True)))(harness.frame_batch(camera, True, device, start, count)))
        sample['render'] += ms
        weights, z_vals = out['weights_fine'].reshape(count, -1), out['z_vals_fine'].reshape(count, -1)
        ms, (offsets, index, points) = event_ms(lambda: ops.select_ray_samples(batch['rays_o_ndc'], batch['rays_d_ndc'], z_vals, weights, 0.0))
        sample['select'] += ms
        ms, grad = event_ms(lambda: model.query_gradient(points, 'fine_mlp')['grad'])
        sample['gradient'] += ms
        ms, (normal[start:start + count], _) = event_ms(lambda: ops.composite_normals(points, grad, offsets, index, weights, parameters))
        sample['composite'] += ms
        rgb[start:start + count], depth[start:start + count] = out['rgb_fine'].reshape(count, 3), out['depth_fine'].reshape(count)
        selected += int(index.shape[0])
        samples += int(weights.numel())
    shown = ops.to_display(rgb, depth)[1].reshape(h, w)
    extrinsic, intrinsic = geometry.camera_matrices(camera)
    sample['depth_normals'], depth_normal = event_ms(lambda: geometry.depth_normals(shown[None], [extrinsic], [intrinsic])[0])
    sample['pictures'], _ = event_ms(lambda: (geometry.normals_to_u8(normal.reshape(h, w, 3), camera), geometry.normals_to_u8(depth_normal, camera)))
    return normal.reshape(h, w, 3), depth_normal, selected, samples


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--precisions', nargs='+', default=('fp32', 'bf16'))
    parser.add_argument('--repeats', type=int, default=3)
    parser.add_argument('--resolution', type=int, nargs=2, default=(756, 1008))
    parser.add_argument('--out', default=None)
    args = parser.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('measure_normals: no GPU; nothing is measured without one')
    camera = synth.camera('fern', 0, resolution=tuple(args.resolution))
    record = {'what': 'the normal maps of one frame (harness.predict_normals) piece by piece, beside harness.predict_frame',
              'device': torch.cuda.get_device_name(0), 'model': 'config2 (NDC, 64 + 128 samples), 8 x 256 / 128 coarse + fine, seeded: a noise field',
              'frame': list(args.resolution), 'ray_block': harness.NORMALS_RAY_BLOCK, 'gradient_block': 1 << 16, 'repeats': args.repeats,
              'note': 'no trained model has been timed; the selected fraction is the seeded noise field\'s', 'runs': []}
    for precision in args.precisions:
        cfg = synth.with_overrides(synth.make_configs('config2'), hip_precision=precision)
        model = get_model(cfg, None)
        shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
        model.load_state_dict({k: torch.from_numpy(v) for k, v in synth.synth_state_dict(shapes, 31, 50.0, 2.0).items()})
        model = model.to(DEV).eval()
        series = {key: [] for key in PIECES + ('predict_normals', 'predict_frame')}
        for repeat in range(args.repeats + 1):                       # (round 0 warms every route)
            sample = dict.fromkeys(series, 0.0)
            normal, depth_normal, selected, samples = one_frame(model, cfg, camera, sample)
            sample['predict_normals'], whole = wall_ms(lambda: harness.predict_normals(model, cfg, camera, torch.device(DEV)))
            assert torch.equal(whole['normal'], normal) and torch.equal(whole['depth_normal'], depth_normal)
            sample['predict_frame'], _ = wall_ms(lambda: harness.predict_frame(model, cfg, camera, torch.device(DEV)))
            if repeat:
                for key in series:
                    series[key].append(sample[key])
            print(f'{precision} round {repeat}: ' + ', '.join(f'{key} {sample[key]:.2f} ms' for key in series), file=sys.stderr, flush=True)
        run = {'precision': precision, 'rays': int(normal.shape[0] * normal.shape[1]), 'samples': samples, 'selected': selected,
               'selected_fraction': selected / samples,
               'rays_with_a_normal': int((whole['normal_strength'] > 0).sum()), 'pixels_with_a_depth_normal': int(depth_normal.any(dim=-1).sum())}
        run.update({f'{key}_event_ms': spread(series[key]) for key in PIECES})
        run.update({f'{key}_ms': spread(series[key]) for key in ('predict_normals', 'predict_frame')})
        run['gradient_points_per_s'] = selected / (statistics.median(series['gradient']) * 1e-3) if selected else None
        record['runs'].append(run)
        del model
        torch.cuda.empty_cache()
    line = json.dumps(record)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
