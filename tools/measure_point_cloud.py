#!/usr/bin/env python3
"""Time the point-cloud export on the device beside a vectorised numpy evaluation of the same rule on the host.  A record, not a gate
(needs the GPU).

    python tools/measure_point_cloud.py [--resolution 756 1008] [--repeats 5] [--voxel 0.05] [--out profiles/point_cloud.json]

The frames are the analytic scene of tests/fuse_reference.py at the given resolution (three cameras, a plane z = 5 in front of a plane
z = 10, depths by ray-plane intersection), generated vectorised here; no model is rendered.  Recorded, each over ``repeats`` rounds
after one warm round:
  fuse_event_ms     HIP events around ``ops.fuse_depth_maps`` (four launches and the read-back of N that narrows the outputs)
  thin_event_ms     HIP events around ``ops.voxel_thin`` of the fused cloud (the bounds' reduction, keys, sort, runs, read-back of M)
  export_wall_ms    wall clock, to a synchronised device, of what ``harness.export_point_cloud`` does after its renders: camera
                    tables on the host, fuse, thin, the copy of the records to the host and the PLY file (a new file each round)
  host_numpy_ms     wall clock of ``fuse_reference.fuse_depth_maps_vectorised`` (numpy float64, one host thread pool as numpy has it)
The kept count of the device is checked against the host's before anything is timed."""
import argparse
import gc
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
from simplenerf_amd import geometry, ops  # noqa: E402
from tests import fuse_reference as ref  # noqa: E402

DEV = 'cuda:0'


def spread(samples):
    return {'median': statistics.median(samples), 'min': min(samples), 'max': max(samples)}


def wall_ms(fn):
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


def event_ms(fn):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    out = fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop), out


def scene(h, w):
    """tests/fuse_reference.scene at (h, w), f = 20 w / 17, without its Python loops."""
    f = 20.0 * w / 17
    poses = [ref.camera_to_world((i - 1.0, 0.1 * i, 0.0), 0.03 * (i - 1)) for i in range(3)]
    intrinsics = numpy.stack([ref.intrinsic_of(h, w, f)] * 3)
    ys, xs = numpy.meshgrid(numpy.arange(h, dtype=numpy.float64), numpy.arange(w, dtype=numpy.float64), indexing='ij')
    pixels = numpy.stack([xs, ys, numpy.ones_like(xs)], axis=-1)
    depth = numpy.empty((3, h, w), dtype=numpy.float32)
    for i, pose in enumerate(poses):
        directions = (pixels @ numpy.linalg.inv(intrinsics[i]).T) @ pose[:3, :3].T
        t = (ref.NEAR_PLANE - pose[2, 3]) / directions[..., 2]
        hit = pose[:3, 3] + t[..., None] * directions
        on_near = (numpy.abs(hit[..., 0]) <= ref.NEAR_HALF_SIDE) & (numpy.abs(hit[..., 1]) <= ref.NEAR_HALF_SIDE)
        depth[i] = numpy.where(on_near, t, (ref.FAR_PLANE - pose[2, 3]) / directions[..., 2])
    return {'depth': depth, 'image': ref.colours_of(3, h, w), 'extrinsics': numpy.stack([numpy.linalg.inv(p) for p in poses]),
            'intrinsics': intrinsics}


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--resolution', type=int, nargs=2, default=(756, 1008))
    parser.add_argument('--repeats', type=int, default=5)
    parser.add_argument('--voxel', type=float, default=0.05)
    parser.add_argument('--tau', type=float, default=0.02)
    parser.add_argument('--min-views', type=int, default=1)
    parser.add_argument('--out', default=None)
    args = parser.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('measure_point_cloud: no GPU; nothing is measured without one')

    h, w = args.resolution
    s = scene(h, w)
    depth, image = torch.from_numpy(s['depth']).to(DEV), torch.from_numpy(s['image']).to(DEV)
    cameras = torch.from_numpy(geometry.fuse_cameras(s['extrinsics'], s['intrinsics'])).to(DEV)
    keep, _, _ = ref.fuse_depth_maps_vectorised(s, args.tau, args.min_views, check_margins=False)
    fused = ops.fuse_depth_maps(depth, image, cameras, args.tau, args.min_views)
    thinned = ops.voxel_thin(fused[0], fused[1], args.voxel)
    # (a pixel decided within rounding of its threshold may differ between host and device at this size: reported, not asserted)
    record = {'what': 'point-cloud export: ops.fuse_depth_maps, ops.voxel_thin and the export after its renders, beside numpy on the host',
              'device': torch.cuda.get_device_name(0), 'host_cpus': os.cpu_count(), 'views': 3, 'resolution': [h, w],
              'pixels': int(depth.numel()), 'depth_error_threshold': args.tau, 'min_views': args.min_views, 'voxel_size': args.voxel,
              'repeats': args.repeats, 'kept': {'device': int(fused[0].shape[0]), 'host_numpy': int(keep.sum())},
              'voxels': int(thinned[0].shape[0]), 'numpy': numpy.__version__}
    root = tempfile.mkdtemp(prefix='measure_point_cloud_')
    counter = [0]

    def export():
        counter[0] += 1
        points, colours, _ = geometry.fuse_depth_maps(depth, image, s['extrinsics'], s['intrinsics'], args.tau, args.min_views)
        points, colours, _ = geometry.voxel_thin(points, colours, args.voxel)
        geometry.save_ply(os.path.join(root, f'{counter[0]:05}.ply'), points, colours)

    def export_unthinned():
        counter[0] += 1
        points, colours, _ = geometry.fuse_depth_maps(depth, image, s['extrinsics'], s['intrinsics'], args.tau, args.min_views)
        geometry.save_ply(os.path.join(root, f'{counter[0]:05}.ply'), points, colours)

    fuse_ms, thin_ms, export_ms, unthinned_ms, host_ms = [], [], [], [], []
    for repeat in range(args.repeats + 1):              # (round 0 warms every route)
        samples = (event_ms(lambda: ops.fuse_depth_maps(depth, image, cameras, args.tau, args.min_views))[0],
                   event_ms(lambda: ops.voxel_thin(fused[0], fused[1], args.voxel))[0], wall_ms(export), wall_ms(export_unthinned),
                   wall_ms(lambda: ref.fuse_depth_maps_vectorised(s, args.tau, args.min_views, check_margins=False)))
        if repeat:
            for series, sample in zip((fuse_ms, thin_ms, export_ms, unthinned_ms, host_ms), samples):
                series.append(sample)
        print(f'round {repeat}: fuse {samples[0]:.3f} ms, thin {samples[1]:.3f} ms, export {samples[2]:.1f} ms, export without thinning '
              f'{samples[3]:.1f} ms, numpy {samples[4]:.1f} ms', file=sys.stderr, flush=True)
    shutil.rmtree(root)
    record.update({'fuse_event_ms': spread(fuse_ms), 'thin_event_ms': spread(thin_ms), 'export_wall_ms': spread(export_ms),
                   'export_without_thinning_wall_ms': spread(unthinned_ms), 'host_numpy_ms': spread(host_ms),
                   'ply_bytes': {'thinned': 15 * int(thinned[0].shape[0]), 'fused': 15 * int(fused[0].shape[0])}})
    line = json.dumps(record)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
