#!/usr/bin/env python3
"""Time the mesh export on the device beside a vectorised numpy evaluation of the integration rule on the host.  A record, not a gate
(needs the GPU).

    python tools/measure_mesh.py [--resolution 756 1008] [--grids 128 256] [--repeats 5] [--out profiles/mesh_export.json]

The frames are three cameras of the analytic scene of tests/mesh_reference.py (a unit sphere, pixels that miss it at depth 8) at
the given resolution, generated vectorised here; no model is rendered.  Per grid of n^3 nodes over [-1.5, 1.5]^3, truncation four
voxels, each over ``repeats`` rounds after one warm round:
  integrate_event_ms  HIP events around ``ops.tsdf_integrate`` (one launch)
  extract_event_ms    HIP events around ``ops.mesh_extract`` (count: five launches; the read-back of the two counts; the allocation
                      of the outputs; emit: one launch)
  colour_event_ms     HIP events around ``ops.colour_points`` of the extracted vertices at a tolerance of one voxel (one launch)
  host_numpy_ms       wall clock of ``mesh_reference.tsdf_integrate_vectorised`` (numpy float64 in slabs of eight layers)
  workspace_bytes     ``snerf_mesh_workspace_bytes``
The device's weights are checked against the host's before anything is timed (a node decided within rounding of a tie may differ at
this size: reported, not asserted)."""
import argparse
import gc
import json
import os
import statistics
import sys
import time

import numpy
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from simplenerf_amd import _lib, geometry, ops  # noqa: E402
from tests import mesh_reference as ref  # noqa: E402

DEV = 'cuda:0'
VIEWS = (0, 2, 4)                   # the cameras on +x, +y and +z


def spread(samples):
    return {'median': statistics.median(samples), 'min': min(samples), 'max': max(samples)}


def wall_ms(fn):
    gc.collect()
    gc.disable()
    try:
        start = time.perf_counter()
        fn()
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
    """Three views of tests/mesh_reference.scene at (h, w), the focal length scaled with the height, without its Python loops."""
    f = ref.SCENE_F * h / ref.SCENE_SIZE
    intrinsic = numpy.array([[f, 0.0, (w - 1) / 2], [0.0, f, (h - 1) / 2], [0.0, 0.0, 1.0]])
    extrinsics = numpy.stack([ref.look_at(ref.SCENE_EYES[v]) for v in VIEWS])
    ys, xs = numpy.meshgrid(numpy.arange(h, dtype=numpy.float64), numpy.arange(w, dtype=numpy.float64), indexing='ij')
    pixels = numpy.stack([xs, ys, numpy.ones_like(xs)], axis=-1)
    depth = numpy.full((len(VIEWS), h, w), ref.SCENE_MISS, dtype=numpy.float32)
    image = numpy.zeros((len(VIEWS), h, w, 3), dtype=numpy.uint8)
    for i, extrinsic in enumerate(extrinsics):
        rotation, eye = extrinsic[:3, :3], -numpy.matmul(extrinsic[:3, :3].T, extrinsic[:3, 3])
        directions = (pixels @ numpy.linalg.inv(intrinsic).T) @ rotation
        a, b, c = (directions * directions).sum(-1), 2 * (directions @ eye), numpy.dot(eye, eye) - 1.0
        root = b * b - 4 * a * c
        hit = root >= 0
        t = (-b - numpy.sqrt(numpy.where(hit, root, 0.0))) / (2 * a)
        depth[i][hit] = t[hit]
        image[i][hit] = numpy.clip(numpy.rint(127.5 + 127.5 * (eye + t[..., None] * directions)), 0, 255)[hit]
    return {'depth': depth, 'image': image, 'extrinsics': extrinsics, 'intrinsics': numpy.stack([intrinsic] * len(VIEWS))}


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--resolution', type=int, nargs=2, default=(756, 1008))
    parser.add_argument('--grids', type=int, nargs='+', default=(128, 256))
    parser.add_argument('--repeats', type=int, default=5)
    parser.add_argument('--out', default=None)
    args = parser.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('measure_mesh: no GPU; nothing is measured without one')

    h, w = args.resolution
    s = scene(h, w)
    depth, image = torch.from_numpy(s['depth']).to(DEV), torch.from_numpy(s['image']).to(DEV)
    cameras = torch.from_numpy(geometry.fuse_cameras(s['extrinsics'], s['intrinsics'])).to(DEV)
    record = {'what': 'mesh export: ops.tsdf_integrate, ops.mesh_extract and ops.colour_points, beside a numpy integration on the host',
              'device': torch.cuda.get_device_name(0), 'host_cpus': os.cpu_count(), 'views': len(VIEWS), 'resolution': [h, w],
              'pixels': int(depth.numel()), 'repeats': args.repeats, 'numpy': numpy.__version__, 'grids': []}
    for n in args.grids:
        lo, voxel, extents = (-1.5, -1.5, -1.5), 3.0 / (n - 1), (n, n, n)
        mu = 4 * voxel
        host = ref.tsdf_integrate_vectorised(s['depth'], s['extrinsics'], s['intrinsics'], lo, voxel, extents, mu)
        tsdf, weight = ops.tsdf_integrate(depth, cameras, lo, voxel, extents, mu)
        vertices, triangles = ops.mesh_extract(tsdf, weight, lo, voxel)
        different = int((weight.cpu().numpy() != host[1]).sum())
        off = float(numpy.abs(tsdf.cpu().numpy() - host[0])[weight.cpu().numpy() == host[1]].max())
        integrate_ms, extract_ms, colour_ms, host_ms = [], [], [], []
        for repeat in range(args.repeats + 1):              # (round 0 warms every route)
            samples = [event_ms(lambda: ops.tsdf_integrate(depth, cameras, lo, voxel, extents, mu))[0],
                       event_ms(lambda: ops.mesh_extract(tsdf, weight, lo, voxel))[0],
                       event_ms(lambda: ops.colour_points(vertices, depth, image, cameras, voxel))[0]]
            if repeat:
                host_ms.append(wall_ms(lambda: ref.tsdf_integrate_vectorised(s['depth'], s['extrinsics'], s['intrinsics'], lo, voxel, extents, mu)))
                for series, sample in zip((integrate_ms, extract_ms, colour_ms), samples):
                    series.append(sample)
            print(f'grid {n}^3 round {repeat}: integrate {samples[0]:.3f} ms, extract {samples[1]:.3f} ms, colour {samples[2]:.3f} ms',
                  file=sys.stderr, flush=True)
        record['grids'].append({'extents': list(extents), 'voxel_size': voxel, 'truncation': mu, 'vertices': int(vertices.shape[0]),
                                'triangles': int(triangles.shape[0]), 'observed_nodes': int((weight > 0).sum()),
                                'weights_unlike_host_numpy': different, 'largest_tsdf_difference_elsewhere': off,
                                'workspace_bytes': int(_lib.load().snerf_mesh_workspace_bytes(*extents)),
                                'ply_bytes': 15 * int(vertices.shape[0]) + 13 * int(triangles.shape[0]),
                                'integrate_event_ms': spread(integrate_ms), 'extract_event_ms': spread(extract_ms),
                                'colour_event_ms': spread(colour_ms), 'host_numpy_ms': spread(host_ms)})
    line = json.dumps(record)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
