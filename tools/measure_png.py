#!/usr/bin/env python3
"""Time the PNG writers: the host writer (``png_encoder='host'``: filter type 0, zlib level 6, one host thread -- the code before the
device encoder existed) against ``png_encoder='device'``.  A record, not a gate (needs the GPU).

    python tools/measure_png.py [--views 16] [--repeats 5] [--resolution 756 1008] [--precision bf16] [--out FILE]   -> one JSON line

One static-camera sweep of a fern frame (756 x 1008, 64 + 128 samples, 8 x 256 coarse + fine, seeded weights) is rendered ONCE;
its V 8-bit frames stay on the device.  Then, alternating host, device, host, device ... for ``repeats`` rounds after one warm round
of each, two writers are timed per route, wall clock from the call to closed files and a synchronised device:
  frames   the V frames as ``predicted_frames/{i:04}.png``: what ``save_static_camera_frames`` does after its render (host: one copy
           of the frames, then ``_png_bytes`` per frame; device: one ``png_files`` call)
  maps     one validation frame's set through ``harness._convert_and_write``: a colour frame and ten grey maps (the sweep's depth,
           depth variance and their NDC forms, twice, and two squared-error maps), PNGs only
Also recorded: the HIP-event time of ``ops.png_deflate`` alone on the V frames, the bytes each route copies to the host for the
frames, and the file sizes of both routes (every device file is inflated and compared with the host route's pixels once)."""
import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

import numpy
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from simplenerf_amd import harness, ops, synth  # noqa: E402
from simplenerf_amd.models.ModelFactory import get_model  # noqa: E402
from tests import png_reference  # noqa: E402

DEV = 'cuda:0'


def spread(samples):
    return {'median': statistics.median(samples), 'min': min(samples), 'max': max(samples)}


def write_frames(frames, directory, encoder):
    os.makedirs(os.path.join(directory, 'predicted_frames'), exist_ok=True)
    if encoder == 'device':
        files = harness.png_files(frames)
    else:
        files = [harness._png_bytes(image) for image in frames.cpu().numpy()]
    for i, data in enumerate(files):
        with open(os.path.join(directory, 'predicted_frames', f'{i:04}.png'), 'wb') as f:
            f.write(data)


def wall_ms(fn):
    torch.cuda.synchronize()
    start = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - start)


def sizes_under(directory):
    return {os.path.relpath(os.path.join(root, name), directory): os.path.getsize(os.path.join(root, name))
            for root, _, names in os.walk(directory) for name in names}


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--views', type=int, default=16)
    parser.add_argument('--repeats', type=int, default=5)
    parser.add_argument('--resolution', type=int, nargs=2, default=None)
    parser.add_argument('--precision', default='bf16', choices=['fp32', 'f16', 'bf16'])
    parser.add_argument('--out', default=None)
    args = parser.parse_args()

    configs = synth.with_overrides(synth.make_configs('config2'), hip_precision=args.precision)
    model = get_model(configs, None)
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    model.load_state_dict({k: torch.from_numpy(v) for k, v in synth.synth_state_dict(shapes, 0, sigma_gain=60.0).items()})
    model = model.to(DEV).eval()
    camera = synth.camera('fern', 0, resolution=args.resolution)
    h, w = camera['resolution']
    rng = numpy.random.RandomState(0)
    view_cameras = []
    for _ in range(args.views):
        c = dict(camera)
        c['pose'] = camera['pose'].copy()
        c['pose'][:3, 3] += (0.3 * rng.standard_normal(3)).astype(numpy.float32)
        view_cameras.append(c)
    swept = harness.predict_view_sweep(model, configs, camera, view_cameras, DEV, keep_device_images=True)
    frames = swept['images_device']
    grey = [torch.from_numpy(swept[name]).to(DEV) for name in ('depth', 'depth_var', 'depth_ndc', 'depth_var_ndc')]
    errors = [((swept['rgb'][0] - swept['rgb'][k]) ** 2).mean(dim=1) for k in (1, 2)]
    maps = [('predicted_frames/0000_fine', swept['rgb'][0].clamp(0, 1), True)]
    maps += [(f'maps/{k:02}', tensor, False) for k, tensor in enumerate(grey + grey + errors)]

    root = tempfile.mkdtemp(prefix='measure_png_')
    writers = {
        'frames': lambda kind: write_frames(frames, os.path.join(root, kind, 'frames'), kind),
        'maps': lambda kind: harness._convert_and_write(maps, (h, w), 0, os.path.join(root, kind, 'maps'), None, write_floats=False, png_encoder=kind),
    }
    wall = {name: {'host': [], 'device': []} for name in writers}
    for repeat in range(args.repeats + 1):          # (round 0 warms both routes)
        for kind in ('host', 'device'):
            for name, writer in writers.items():
                ms = wall_ms(lambda: writer(kind))
                if repeat:
                    wall[name][kind].append(ms)
        print(f'round {repeat}: ' + ', '.join(f'{name} {kind} {wall[name][kind][-1]:.1f} ms' for name in writers for kind in ('host', 'device')
                                              if wall[name][kind]), file=sys.stderr, flush=True)

    kernel = []
    for _ in range(args.repeats + 1):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        _, stream_sizes = ops.png_deflate(frames)
        stop.record()
        stop.synchronize()
        kernel.append(start.elapsed_time(stop))
    host_files, device_files = sizes_under(os.path.join(root, 'host')), sizes_under(os.path.join(root, 'device'))
    assert sorted(host_files) == sorted(device_files)
    for name in host_files:          # the two routes' files hold the same pixels
        with open(os.path.join(root, 'host', name), 'rb') as f, open(os.path.join(root, 'device', name), 'rb') as g:
            data, height, width, bpp = png_reference.inflate(f.read())          # (the host writer's rows are unfiltered)
            pixels = numpy.frombuffer(data, dtype=numpy.uint8).reshape(height, 1 + width * bpp)[:, 1:]
            assert png_reference.holds(g.read(), pixels.reshape((height, width, 3) if bpp == 3 else (height, width))), name
    shutil.rmtree(root)

    def total(files, part):
        return sum(size for name, size in files.items() if name.startswith(part))

    raw_frames = args.views * h * w * 3
    record = {'what': "PNG writers: png_encoder='host' (the code before the device encoder) against 'device'", 'device': torch.cuda.get_device_name(0),
              'host_cpus': os.cpu_count(), 'resolution': [h, w], 'views': args.views, 'precision': args.precision, 'repeats': args.repeats,
              'wall_ms': {name: {kind: spread(samples) for kind, samples in kinds.items()} for name, kinds in wall.items()},
              'ratio': {name: statistics.median(kinds['host']) / statistics.median(kinds['device']) for name, kinds in wall.items()},
              'png_deflate_event_ms': spread(kernel[1:]),
              'frames_d2h_bytes': {'host': raw_frames, 'device': int(stream_sizes.sum().item()) + 8 * args.views},
              'file_bytes': {part: {'raw_pixels': raw_frames if part == 'frames' else (3 + 10) * h * w,
                                    'host': total(host_files, part), 'device': total(device_files, part)} for part in ('frames', 'maps')}}
    line = json.dumps(record)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
