#!/usr/bin/env python3
"""Time the JPEG / Motion-JPEG writers on the device against PIL's encoder on the host.  A record, not a gate (needs the GPU and PIL).

    python tools/measure_jpeg.py [--views 16] [--repeats 5] [--resolution 756 1008] [--precision bf16] [--quality 90] [--out FILE]

Two sets of V frames of the same size, each named in the record:
  sweep      one static-camera sweep of a fern frame (756 x 1008, 64 + 128 samples, 8 x 256 coarse + fine, SEEDED weights), rendered
             once; its 8-bit frames stay on the device.  Seeded-weight frames are nearly flat: a few bits per block.
  textured   tests/jpeg_reference.textured: stripes, ramps and seeded noise -- many coefficients per block, as a photograph has.
Per set, alternating host, device, ... for ``repeats`` rounds after one warm round of each, wall clock to a synchronised device:
  jpeg_files   device: ``harness.jpeg_files(frames)``; host: one copy of the frames, then PIL (``quality``, ``subsampling=2``,
               ``optimize=False``, one host thread) per frame
  save_video   device: ``harness.save_video`` to a new file; host: the host route's files through the same AVI writer to a new file
Also recorded: the HIP-event time of ``ops.jpeg_scan`` alone, the bytes each route copies to the host, the file sizes, the PSNR of
PIL's decode of both routes' first frame, and the restated encoder's margins against PIL (the figures of tests/test_jpeg_host.py)."""
import argparse
import gc
import io
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

import numpy
import torch
import PIL
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from simplenerf_amd import harness, ops, synth  # noqa: E402
from simplenerf_amd.models.ModelFactory import get_model  # noqa: E402
from tests import jpeg_reference, png_reference  # noqa: E402

DEV = 'cuda:0'


def spread(samples):
    return {'median': statistics.median(samples), 'min': min(samples), 'max': max(samples)}


def wall_ms(fn):
    """Wall clock of ``fn`` to a synchronised device, with the cyclic garbage collector off as ``timeit`` has it: a collection
    that walks the model's object graph costs more than the device route takes."""
    torch.cuda.synchronize()
    gc.collect()
    gc.disable()
    try:
        start = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - start)
    finally:
        gc.enable()


def pil_file(image, quality):
    blob = io.BytesIO()
    Image.fromarray(image).save(blob, 'JPEG', quality=quality, subsampling=2, optimize=False)
    return blob.getvalue()


def pil_decode(blob):
    with Image.open(io.BytesIO(blob)) as opened:
        return numpy.asarray(opened)


def host_files(frames, quality):
    return [pil_file(image, quality) for image in frames.cpu().numpy()]


def margins():
    """The restated encoder against PIL on the six 96 x 128 fixtures of tests/test_jpeg_host.py."""
    fixtures = {'smooth': png_reference.smooth(96, 128), 'textured': jpeg_reference.textured(96, 128), 'noise': jpeg_reference.noise(96, 128),
                'smooth grey': png_reference.smooth(96, 128, 1), 'textured grey': jpeg_reference.textured(96, 128, 1),
                'noise grey': jpeg_reference.noise(96, 128, 1)}
    rows = {}
    for name, image in fixtures.items():
        for quality in (50, 90):
            ours, theirs = jpeg_reference.encode(image, quality), pil_file(image, quality)
            channels = 3 if image.ndim == 3 else 1
            structure = 6 + jpeg_reference.geometry(96, 128, channels)[2] * (3 + (8 if channels == 3 else 3)) - 2
            row = {'psnr_db': {'ours': jpeg_reference.psnr(pil_decode(ours), image), 'pil': jpeg_reference.psnr(pil_decode(theirs), image)},
                   'bytes': {'ours': len(ours), 'pil': len(theirs), 'structure': structure},
                   'size_excess': (len(ours) - structure - len(theirs)) / len(theirs)}
            if channels == 1:
                mine, pil = jpeg_reference.parse(ours), jpeg_reference.parse(theirs)
                exact = jpeg_reference.exact_levels(jpeg_reference.planes(image)[0], mine['quant'][0])
                row['levels_differing_from_exact'] = {'ours': float(numpy.mean(mine['levels'][0] != exact)),
                                                      'pil': float(numpy.mean(pil['levels'][0] != exact))}
            rows[f'{name}, quality {quality}'] = row
    return {'fixtures': rows,
            'largest_psnr_shortfall_db': max(r['psnr_db']['pil'] - r['psnr_db']['ours'] for r in rows.values()),
            'largest_size_excess': max(r['size_excess'] for r in rows.values()),
            'largest_level_share_excess': max(r['levels_differing_from_exact']['ours'] - r['levels_differing_from_exact']['pil']
                                              for r in rows.values() if 'levels_differing_from_exact' in r)}


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--views', type=int, default=16)
    parser.add_argument('--repeats', type=int, default=5)
    parser.add_argument('--resolution', type=int, nargs=2, default=None)
    parser.add_argument('--precision', default='bf16', choices=['fp32', 'f16', 'bf16'])
    parser.add_argument('--quality', type=int, default=90)
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
    contents = {
        'sweep': ('the frames of a static-camera sweep of a model with seeded weights: nearly flat', swept['images_device']),
        'textured': ('tests/jpeg_reference.textured: stripes, ramps and seeded noise',
                     torch.from_numpy(numpy.stack([jpeg_reference.textured(h, w, seed=s) for s in range(args.views)])).to(DEV)),
    }
    root = tempfile.mkdtemp(prefix='measure_jpeg_')
    counter = [0]

    def new_path():
        counter[0] += 1
        return os.path.join(root, f'{counter[0]:05}.avi')

    def host_video(frames):
        data = harness._avi_bytes(host_files(frames, args.quality), h, w, harness.VIDEO_FRAME_RATE)
        with open(new_path(), 'wb') as f:
            f.write(data)

    record = {'what': 'JPEG frames and Motion-JPEG AVI: the device encoder (harness.jpeg_files, save_video) against PIL on the host',
              'device': torch.cuda.get_device_name(0), 'host_cpus': os.cpu_count(), 'resolution': [h, w], 'views': args.views,
              'precision': args.precision, 'quality': args.quality, 'repeats': args.repeats, 'pil': PIL.__version__,
              'contents': {}}
    for name, (described, frames) in contents.items():
        writers = {
            'jpeg_files': {'device': lambda: harness.jpeg_files(frames, args.quality), 'host': lambda: host_files(frames, args.quality)},
            'save_video': {'device': lambda: harness.save_video(new_path(), frames, quality=args.quality), 'host': lambda: host_video(frames)},
        }
        wall = {what: {'host': [], 'device': []} for what in writers}
        for repeat in range(args.repeats + 1):          # (round 0 warms both routes)
            for kind in ('host', 'device'):
                for what, routes in writers.items():
                    ms = wall_ms(routes[kind])
                    if repeat:
                        wall[what][kind].append(ms)
            print(f'{name} round {repeat}: ' + ', '.join(f'{what} {kind} {wall[what][kind][-1]:.1f} ms' for what in writers for kind in ('host', 'device')
                                                        if wall[what][kind]), file=sys.stderr, flush=True)
        kernel = []
        for _ in range(args.repeats + 1):
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            _, scan_sizes = ops.jpeg_scan(frames, args.quality)
            stop.record()
            stop.synchronize()
            kernel.append(start.elapsed_time(stop))
        ours, theirs = harness.jpeg_files(frames, args.quality), host_files(frames, args.quality)
        first = frames[0].cpu().numpy()
        record['contents'][name] = {
            'frames': described,
            'wall_ms': {what: {kind: spread(samples) for kind, samples in kinds.items()} for what, kinds in wall.items()},
            'host_over_device': {what: statistics.median(kinds['host']) / statistics.median(kinds['device']) for what, kinds in wall.items()},
            'jpeg_scan_event_ms': spread(kernel[1:]),
            'd2h_bytes': {'host': args.views * h * w * 3, 'device': int(scan_sizes.sum().item()) + 8 * args.views},
            'file_bytes': {'raw_pixels': args.views * h * w * 3, 'device': sum(len(f) for f in ours), 'host': sum(len(f) for f in theirs)},
            'first_frame_psnr_db': {'device': jpeg_reference.psnr(pil_decode(ours[0]), first), 'host': jpeg_reference.psnr(pil_decode(theirs[0]), first)},
        }
    shutil.rmtree(root)
    record['restated_encoder_against_pil'] = margins()
    line = json.dumps(record)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
