#!/usr/bin/env python3
"""Time the visibility mask of ONE 756 x 1008 test frame against 3 training views on the device -- every stage and the whole of
``qa.visibility_mask`` -- and with the host restatement the tests use (tests/mask_reference.py: numpy) on the same box.  A record,
not a gate.
    python tools/measure_masks.py [repeats] [--sorter torch|library]      -> one JSON line
stage_ms / device_ms: HIP events around what the stage / the whole call enqueues (project + the fold of its maxima, the stable
sort of the keys -- torch's or, with ``--sorter library``, the HIP library's -- the list starts, gather with the depth test,
combine), warm, median of ``repeats`` (default 25); call_ms: a host
clock around the call, matrices inverted on the host and copied, to the synchronised mask; host_ms: the restatement, median of 3.
The scene is the analytic occlusion scene of the fixtures (a sphere in front of a slanted plane) at that resolution."""
import json
import os
import statistics
import sys
import time

import numpy
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from simplenerf_amd import ops, qa  # noqa: E402
from tests import mask_reference  # noqa: E402

DEV = torch.device('cuda', 0)
KEYS = ('extrinsics_train', 'extrinsic_test', 'intrinsics_train', 'intrinsic_test')


def timed(stages, name, call):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    out = call()
    stop.record()
    stages.setdefault(name, []).append((start, stop))
    return out


def enqueue(depth_train, depth_test, cameras, stages, sorter='torch'):
    """What qa.visibility_mask puts on the stream, stage by stage."""
    views, h, w = depth_train.shape
    points, keys, stats = timed(stages, 'project', lambda: ops.visibility_mask_project(depth_train, cameras))
    if sorter == 'library':
        key_bits = (views * ((h + 1) * (w + 1) + 1) - 1).bit_length()
        sorted_keys, order = timed(stages, 'sort', lambda: ops.sort_keys_with_order(keys.reshape(-1), key_bits))
    else:
        sorted_keys, order = timed(stages, 'sort', lambda: torch.sort(keys.reshape(-1), stable=True))
    starts = timed(stages, 'list_starts', lambda: ops.visibility_mask_list_starts(sorted_keys, views, h, w))
    mask_views = timed(stages, 'gather', lambda: ops.visibility_mask_gather(points, order, starts, stats, depth_test, 0.05))
    return timed(stages, 'combine', lambda: ops.visibility_mask_combine(mask_views, 2))


def main():
    args = sys.argv[1:]
    sorter = args.pop(args.index('--sorter') + 1) if '--sorter' in args else 'torch'
    args = [a for a in args if a != '--sorter']
    qa._sorter(sorter)
    repeats = int(args[0]) if args else 25
    scene = mask_reference.occlusion_scene(756, 1008, 'generic')
    depth_train, depth_test = torch.as_tensor(scene['depth_train']).to(DEV), torch.as_tensor(scene['depth_test']).to(DEV)
    cameras = torch.from_numpy(qa.visibility_cameras(*(scene[k] for k in KEYS))).to(DEV)
    for _ in range(5):
        enqueue(depth_train, depth_test, cameras, {}, sorter)
    torch.cuda.synchronize()
    stages, whole, call_ms = {}, [], []
    for _ in range(repeats):
        mask = timed(stages, 'whole', lambda: enqueue(depth_train, depth_test, cameras, stages, sorter))
    torch.cuda.synchronize()
    stage_ms = {name: statistics.median(a.elapsed_time(b) for a, b in events) for name, events in stages.items()}
    whole = [a.elapsed_time(b) for a, b in stages['whole']]
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        mask = qa.visibility_mask(depth_train, depth_test, *(scene[k] for k in KEYS), sorter=sorter)
        torch.cuda.synchronize()
        call_ms.append(1e3 * (time.perf_counter() - t0))
    host_ms = []
    for _ in range(3):
        t0 = time.perf_counter()
        want = mask_reference.visibility_mask(scene['depth_train'], scene['depth_test'], *(scene[k] for k in KEYS))
        host_ms.append(1e3 * (time.perf_counter() - t0))
    got = qa.visibility_mask(depth_train, depth_test, *(scene[k] for k in KEYS), return_views=True, sorter=sorter)
    got = dict(zip(('mask', 'mask_views', 'warped_depth', 'weight_sum'), (t.cpu().numpy() for t in got)))
    got['warping_mask'] = got['weight_sum'] > 0
    # masks are held to the restatement on every pixel; warped_depth is REPORTED, not gated: at this width a position near 1000 carries
    # a few ulps (4.5e-13 between two fp64 evaluations of the projection), which a small proximity weight at an occlusion edge
    # amplifies -- two host evaluations that differ only in the order of the 3x3 products already differ by 3e-12 here, and either
    # differs from the reference itself by 1.5e-12; the 1e-12 gate of the tests belongs to their shapes
    figures = mask_reference.compare(got, want, scene['depth_test'], [0.05 * float(d.max()) for d in scene['depth_train']], float('inf'))
    assert numpy.array_equal(mask.cpu().numpy(), got['mask'])
    del stage_ms['whole']
    print(json.dumps({'what': 'visibility mask of one 756x1008 test frame from 3 training views', 'repeats': repeats,
                      'sorter': sorter, 'device_ms_median': statistics.median(whole), 'device_ms_min': min(whole), 'device_ms_max': max(whole),
                      'stage_ms_median': stage_ms, 'call_ms_median': statistics.median(call_ms),
                      'host_restatement_ms_median': statistics.median(host_ms), 'host_threads': torch.get_num_threads(),
                      'visible': float(got['mask'].mean()), 'warped': float(got['warping_mask'].mean()), 'against_restatement': figures}))


if __name__ == '__main__':
    main()
