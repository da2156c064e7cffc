#!/usr/bin/env python3
"""Time the density-mesh export on the device, launch by launch, beside the depth-map mesh export of the same cameras.  A record, not
a gate (needs the GPU).

    python tools/measure_field.py [--resolution 756 1008] [--grids 128 256] [--precisions fp32 bf16] [--repeats 3]
                                  [--out profiles/density_mesh.json]

The model is the seeded 8 x 256 / 128 coarse + fine NDC model of ``synth.make_configs('config2')`` (weights of
``synth.synth_state_dict(shapes, 31, 50.0, 2.0)``), the cameras three poses of the fern scene at the given resolution.  Per precision
and grid of n^3 nodes over the box [-1.5, 1.5] x [-1.5, 1.5] x [-4.2, -1.2] of the scene frame, the level the median of the positive
densities of a 32^3 probe, blocks of 2^20 points, each over ``repeats`` rounds after one warm round:
  grid_points_event_ms   HIP events around every ``ops.field_grid_points`` block, summed over the grid (one launch a block)
  mlp_event_ms           HIP events around every ``model.query`` block (the S = 1 shape of the forward kernels), summed
  mlp_points_per_s       nodes / that time
  values_event_ms        HIP events around ``ops.field_values`` (one launch)
  extract_event_ms       HIP events around ``ops.mesh_extract``
  point_views_event_ms   HIP events around ``ops.field_point_views`` of the extracted vertices (one launch)
  colour_mlp_event_ms    HIP events around ``model.query`` with those directions, and ``ops.to_display``
  export_event_ms        HIP events around the whole ``harness.export_density_mesh`` (a fresh file each round, its write included)
  render_export_event_ms HIP events around ``harness.export_mesh`` over the same box at the same voxel size: V full-frame renders, the
                         TSDF, the extraction, the colours, the file"""
import argparse
import json
import os
import statistics
import sys
import tempfile

import numpy
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from simplenerf_amd import geometry, harness, ops, synth  # noqa: E402
from simplenerf_amd.models.ModelFactory import get_model  # noqa: E402

DEV = 'cuda:0'
BOX = ((-1.5, -1.5, -4.2), (1.5, 1.5, -1.2))
BLOCK = 1 << 20


def spread(samples):
    return {'median': statistics.median(samples), 'min': min(samples), 'max': max(samples)}


def event_ms(fn):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    out = fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop), out


def seeded_model(precision):
    cfg = synth.with_overrides(synth.make_configs('config2'), hip_precision=precision)
    model = get_model(cfg, None)
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    model.load_state_dict({k: torch.from_numpy(v) for k, v in synth.synth_state_dict(shapes, 31, 50.0, 2.0).items()})
    return cfg, model.to(DEV).eval()


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--resolution', type=int, nargs=2, default=(756, 1008))
    parser.add_argument('--grids', type=int, nargs='+', default=(128, 256))
    parser.add_argument('--precisions', nargs='+', default=('fp32', 'bf16'))
    parser.add_argument('--repeats', type=int, default=3)
    parser.add_argument('--out', default=None)
    args = parser.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('measure_field: no GPU; nothing is measured without one')

    resolution = tuple(args.resolution)
    cameras = [synth.camera('fern', pose, resolution=resolution) for pose in (0, 1, 2)]
    matrices = [geometry.camera_matrices(camera) for camera in cameras]
    extrinsics, intrinsics = [m[0] for m in matrices], [m[1] for m in matrices]
    table = torch.from_numpy(geometry.fuse_cameras(numpy.stack(extrinsics), numpy.stack(intrinsics))).to(DEV)
    ndc = geometry.ndc_parameters(cameras[0])
    device = torch.device(DEV)
    record = {'what': 'density-mesh export (harness.export_density_mesh) launch by launch, beside harness.export_mesh of the same cameras',
              'device': torch.cuda.get_device_name(0), 'model': 'config2, 8 x 256 / 128 coarse + fine, NDC, seeded', 'views': len(cameras),
              'resolution': list(resolution), 'box': [list(BOX[0]), list(BOX[1])], 'point_block': BLOCK, 'repeats': args.repeats, 'runs': []}
    with tempfile.TemporaryDirectory() as tmp:
        for precision in args.precisions:
            cfg, model = seeded_model(precision)
            probe = ops.field_grid_points(BOX[0], 3.0 / 31, (32, 32, 32), table, resolution, ndc)[0]
            densities = model.query(probe)['sigma']
            level = float(densities[densities > 0].median())
            for n in args.grids:
                voxel, extents = 3.0 / (n - 1), (n, n, n)
                nodes = n ** 3
                series = {key: [] for key in ('grid_points', 'mlp', 'values', 'extract', 'point_views', 'colour_mlp', 'export', 'render_export')}
                for repeat in range(args.repeats + 1):              # (round 0 warms every route)
                    sample = dict.fromkeys(series, 0.0)
                    sigma = torch.empty((nodes,), dtype=torch.float32, device=DEV)
                    weight = torch.empty((nodes,), dtype=torch.uint8, device=DEV)
                    for first in range(0, nodes, BLOCK):
                        count = min(BLOCK, nodes - first)
                        ms, (points, weight[first:first + count]) = event_ms(
                            lambda: ops.field_grid_points(BOX[0], voxel, extents, table, resolution, ndc, first, count))
                        sample['grid_points'] += ms
                        ms, out = event_ms(lambda: model.query(points, point_block=BLOCK))
                        sample['mlp'] += ms
                        sigma[first:first + count] = out['sigma']
                    sample['values'], tsdf = event_ms(lambda: ops.field_values(sigma, weight, level))
                    tsdf, weight = tsdf.reshape(n, n, n), weight.reshape(n, n, n)
                    sample['extract'], (vertices, triangles) = event_ms(lambda: ops.mesh_extract(tsdf, weight, BOX[0], voxel))
                    sample['point_views'], (mlp_points, dirs, views) = event_ms(lambda: ops.field_point_views(vertices, table, resolution, ndc))
                    sample['colour_mlp'], colours = event_ms(lambda: ops.to_display(model.query(mlp_points, dirs, point_block=BLOCK)['rgb'])[0])
                    path = os.path.join(tmp, f'density_{precision}_{n}_{repeat}.ply')
                    sample['export'], whole = event_ms(
                        lambda: harness.export_density_mesh(model, cfg, cameras, path, device, voxel, level, (BOX[0], [b - 1e-9 for b in BOX[1]])))
                    assert whole['extents'] == extents and torch.equal(whole['vertices'], vertices) and torch.equal(whole['colours'], colours)
                    path = os.path.join(tmp, f'render_{precision}_{n}_{repeat}.ply')
                    sample['render_export'], rendered = event_ms(
                        lambda: harness.export_mesh(model, cfg, cameras, path, device, voxel, bounds=(BOX[0], [b - 1e-9 for b in BOX[1]])))
                    if repeat:
                        for key in series:
                            series[key].append(sample[key])
                    print(f'{precision} grid {n}^3 round {repeat}: ' + ', '.join(f'{key} {sample[key]:.2f} ms' for key in series),
                          file=sys.stderr, flush=True)
                    del whole
                run = {'precision': precision, 'extents': list(extents), 'voxel_size': voxel, 'level': level, 'nodes': nodes,
                       'seen_nodes': int((weight > 0).sum()), 'vertices': int(vertices.shape[0]), 'triangles': int(triangles.shape[0]),
                       'coloured_from_a_view': int((views != ops.FIELD_NO_VIEW).sum()),
                       'render_export_vertices': int(rendered['vertices'].shape[0]), 'render_export_triangles': int(rendered['triangles'].shape[0]),
                       'mlp_points_per_s': nodes / (statistics.median(series['mlp']) * 1e-3)}
                run.update({f'{key}_event_ms': spread(samples) for key, samples in series.items()})
                record['runs'].append(run)
                del rendered
    line = json.dumps(record)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
