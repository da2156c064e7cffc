#!/usr/bin/env python3
"""Time the scoring of ONE 756 x 1008 frame (image + depth, with a mask) on the device and with the host restatement the tests
use (tests/qa_reference.py: numpy + scipy) on the same box.  A record, not a gate.
    python tools/measure_qa.py [repeats] [--sorter torch|library]      -> one JSON line
device_ms: HIP events around everything ``qa.image_metrics`` + ``qa.depth_metrics`` enqueue (the error sums, SSIM plain and
masked, four sorts, the mask compaction, the rank sums -- sorts and compaction by torch or, with ``--sorter library``, by the HIP
library), warm, median of ``repeats`` (default 25); call_ms: a host clock around the
two calls, which end in the copy of their scalars to the host; host_ms: the restatement, median of 3."""
import json
import os
import statistics
import sys
import time

import numpy
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from simplenerf_amd import ops, qa  # noqa: E402
from tests import qa_reference  # noqa: E402

DEV = torch.device('cuda', 0)


def frame(h=756, w=1008, seed=0):
    rng = numpy.random.default_rng(seed)
    y, x = numpy.mgrid[0:h, 0:w]
    gt = numpy.clip(128 + 90 * (numpy.sin(x / 23) * numpy.cos(y / 31))[..., None] + rng.normal(0, 12, (h, w, 3)), 0, 255).astype(numpy.uint8)
    image = numpy.clip(gt + rng.normal(0, 6, (h, w, 3)), 0, 255).astype(numpy.uint8)
    gt_depth = (3 + numpy.sin(x / 40) + 0.5 * numpy.cos(y / 17) + rng.normal(0, 0.05, (h, w))).astype(numpy.float32)
    depth = numpy.maximum(gt_depth * 1.1 + rng.normal(0, 0.2, (h, w)) - 2.2, 0).astype(numpy.float32)
    return gt, image, gt_depth, depth, rng.random((h, w)) < 0.7


def enqueue(gt, image, gt_depth, depth, mask, sorter='torch'):
    """What the two qa calls put on the stream, without their copy to the host."""
    sort = ops.sort_values if sorter == 'library' else (lambda v: torch.sort(v).values)
    ops.image_error_sums(gt, image, mask)
    ops.ssim_sums(gt, image)
    ops.ssim_sums(gt, image, mask)
    g, e = gt_depth.reshape(-1), depth.reshape(-1)
    sorted_gt = sort(g)
    ops.depth_error_sums(gt_depth, depth, 1.0, 1.0, None, sorted_gt)
    ops.rank_correlation_sums(g, e, sorted_gt, sort(e))
    ops.depth_error_sums(gt_depth, depth, 1.0, 1.0, mask)
    keep = mask.reshape(-1)
    gm, em = ops.compact_pair(g, e, keep) if sorter == 'library' else (g[keep], e[keep])
    ops.rank_correlation_sums(gm, em, sort(gm), sort(em))


def main():
    args = sys.argv[1:]
    sorter = args.pop(args.index('--sorter') + 1) if '--sorter' in args else 'torch'
    args = [a for a in args if a != '--sorter']
    qa._sorter(sorter)
    repeats = int(args[0]) if args else 25
    host = frame()
    on_device = [torch.as_tensor(a).to(DEV) for a in host]
    gt, image, gt_depth, depth, mask = on_device
    for _ in range(5):
        enqueue(*on_device, sorter)
    torch.cuda.synchronize()
    device_ms, call_ms = [], []
    for _ in range(repeats):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        enqueue(*on_device, sorter)
        stop.record()
        stop.synchronize()
        device_ms.append(start.elapsed_time(stop))
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = qa.image_metrics(image, gt, mask)
        got.update(qa.depth_metrics(depth, gt_depth, mask=mask, sorter=sorter))
        call_ms.append(1e3 * (time.perf_counter() - t0))
    host_ms = []
    for _ in range(3):
        t0 = time.perf_counter()
        want = qa_reference.image_metrics(host[1], host[0], host[4])
        want.update(qa_reference.depth_metrics(host[3], host[2], mask=host[4]))
        host_ms.append(1e3 * (time.perf_counter() - t0))
    qa_reference.assert_close(got, want)
    print(json.dumps({'what': 'score one 756x1008 frame: RMSE/PSNR/SSIM + depth RMSE/MAE/SROCC, plain and masked', 'repeats': repeats,
                      'sorter': sorter, 'device_ms_median': statistics.median(device_ms), 'device_ms_min': min(device_ms), 'device_ms_max': max(device_ms),
                      'call_ms_median': statistics.median(call_ms), 'host_restatement_ms_median': statistics.median(host_ms),
                      'host_threads': torch.get_num_threads(), 'PSNR': got['PSNR'], 'SSIM': got['SSIM']}))


if __name__ == '__main__':
    main()
