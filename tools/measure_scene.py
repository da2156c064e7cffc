#!/usr/bin/env python3
"""Time the scene stage, raw loader data -> first training batch ready, at the LLFF size: 3 views of 756 x 1008, 1000 sparse-depth
points per view, NDC (``synth.raw_scene``).  A record, not a gate.
    python tools/measure_scene.py [repeats]                  -> one JSON line (needs the GPU)
    python tools/measure_scene.py [repeats] --reference SRC  -> one JSON line: the REFERENCE's DataPreprocessor constructor and first
                                                                batch on the same raw data, on this machine's CPU (SRC = the src/
                                                                directory of a checkout of the reference; skimage stubbed, pandas
                                                                needed; no GPU)
GPU side, per repeat (median of ``repeats``, default 9, after two warm runs): ``device_ms`` = HIP events around everything the
constructor and the first ``get_next_batch`` enqueue (uploads of the raw arrays included), ``wall_ms`` = host clock around the same
up to the synchronisation after the batch, ``host_prepare_ms`` = the host part alone (poses, point concatenation), and the three
scene kernels on their own with their inputs already on the device."""
import json
import os
import statistics
import sys
import time
import types

import numpy

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from simplenerf_amd import synth  # noqa: E402

H, W, VIEWS, POINTS = 756, 1008, 3, 1000
CONFIGS = {'data_loader': {'bd_factor': 0.75, 'batching': True, 'ndc': True, 'downsampling_factor': 1, 'num_rays': 2048,
                           'recenter_camera_poses': True, 'spherify': False, 'precrop_iterations': 0, 'sparse_depth': {'num_rays': 2048}},
           'model': {'white_bkgd': False}, 'device': [0], 'seed': 0}


def reference_side(src, repeats):
    import copy
    import pandas
    sys.path.insert(0, src)
    for name in ('skimage', 'skimage.io', 'skimage.transform'):
        sys.modules.setdefault(name, types.ModuleType(name))
    from data_preprocessors.DataPreprocessor01 import DataPreprocessor
    raw = synth.raw_scene(0, VIEWS, H, W, POINTS)
    configs = dict(CONFIGS, device='cpu')
    build, first = [], []
    for _ in range(repeats):
        data = copy.deepcopy(raw)
        data['sparse_depth_data'] = {f: pandas.DataFrame(t) for f, t in data['sparse_depth_data'].items()}
        numpy.random.seed(0)
        t0 = time.perf_counter()
        pp = DataPreprocessor(configs, mode='train', raw_data_dict=data)
        t1 = time.perf_counter()
        pp.get_next_batch(0)
        t2 = time.perf_counter()
        build.append(1e3 * (t1 - t0))
        first.append(1e3 * (t2 - t1))
    return {'what': "the reference's DataPreprocessor on the same raw data, CPU only (another machine than the GPU figures)",
            'repeats': repeats, 'constructor_ms_median': statistics.median(build), 'constructor_ms_min': min(build),
            'first_batch_ms_median': statistics.median(first), 'cpu_threads': os.cpu_count()}


def device_side(repeats):
    import torch
    from simplenerf_amd import ops
    from simplenerf_amd.data_preprocessors import DataPreprocessor01 as dp
    dev = torch.device('cuda', 0)
    raw = synth.raw_scene(0, VIEWS, H, W, POINTS)

    def event_ms(call):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        call()
        stop.record()
        stop.synchronize()
        return start.elapsed_time(stop)

    def whole():
        pp = dp.DataPreprocessor(CONFIGS, 'train', raw, device=dev)
        return pp.get_next_batch(0)

    device, wall, host = [], [], []
    for i in range(repeats + 2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ms = event_ms(whole)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        dp.prepare_host(CONFIGS, raw)
        t2 = time.perf_counter()
        if i >= 2:
            device.append(ms)
            wall.append(1e3 * (t1 - t0))
            host.append(1e3 * (t2 - t1))
    pp = dp.DataPreprocessor(CONFIGS, 'train', raw, device=dev)
    points = {k: torch.from_numpy(v).to(dev) for k, v in dp.collect_points(raw).items()}
    images = torch.from_numpy(raw['nerf_data']['images']).to(dev)
    table = ops.camera_table(pp.scene['intrinsics'], pp.scene['poses'], (H, W))
    sc = pp.get_model_configs()['translation_scale']
    kernels = {
        'scene_images': lambda: ops.scene_images(images),
        'rasterise_sparse_depth_with_ndc': lambda: ops.rasterise_sparse_depth(points['x'], points['y'], points['depth'],
                                                                              points['reprojection_error'], points['view'], VIEWS, (H, W),
                                                                              scale=sc, table=table),
        'depth_table_to_ndc': lambda: ops.depth_table_to_ndc(pp.scene['sparse_depths'], table, (H, W), 1.0),
    }
    out = {}
    for name, call in kernels.items():
        for _ in range(3):
            call()
        out[f'{name}_ms_median'] = statistics.median(event_ms(call) for _ in range(max(repeats, 9)))
    return {'what': f'raw loader data -> first training batch, {VIEWS} x {H} x {W}, {POINTS} points per view, NDC', 'repeats': repeats,
            'device_ms_median': statistics.median(device), 'device_ms_min': min(device), 'device_ms_max': max(device),
            'wall_ms_median': statistics.median(wall), 'wall_ms_min': min(wall), 'host_prepare_ms_median': statistics.median(host),
            'sparse_pixels': int((pp.scene['sparse_depths'] > 0).sum()), **out}


def main():
    args = sys.argv[1:]
    src = args.pop(args.index('--reference') + 1) if '--reference' in args else None
    args = [a for a in args if a != '--reference']
    repeats = int(args[0]) if args else 9
    print(json.dumps(reference_side(src, repeats) if src else device_side(repeats)))


if __name__ == '__main__':
    main()
