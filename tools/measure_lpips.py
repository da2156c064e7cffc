#!/usr/bin/env python3
"""Time LPIPS of ONE 756 x 1008 frame pair with a mask (LPIPS + MaskedLPIPS: two passes of the network over two images each) on the
device, and the float32 torch restatement the tests use (tests/lpips_reference.py) on the same box's CPU threads.  A record, not a
gate.  Random weights (lpips_reference.random_weights): the arithmetic does not depend on their values.
    python tools/measure_lpips.py [repeats]          -> one JSON line
    python tools/measure_lpips.py --kernels [calls]  -> only `calls` (default 10) warm ops.lpips_sums calls, for a run under
                                                        rocprofv3 --kernel-trace --stats (the per-kernel times; every layer's
                                                        convolution is its own instantiation conv_relu_kernel<layer>)
device_ms: HIP events around what ONE ``ops.lpips_sums`` enqueues (prepare, five convolutions, two pools, five layer reductions,
the fold), warm, median of ``repeats`` (default 25); call_ms: a host clock around ``qa.lpips_metrics`` with the mask (two such
passes and the copy of ten scalars to the host); host_ms: the float32 restatement of one pass, median of 3.
conv_fraction_of_fp32_matrix_peak counts 2 x 10.8 GMAC = 43.4 GFLOP per pass against device_ms (an upper bound on the convolutions'
time: the other kernels are inside it) and the MI355X's 157.3 TFLOP/s fp32 matrix peak."""
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from simplenerf_amd import ops, qa  # noqa: E402
from tests import lpips_reference  # noqa: E402

DEV = torch.device('cuda', 0)
FP32_MATRIX_PEAK = 157.3e12


def conv_flops(h, w):
    """2 x multiply-accumulates of the five convolutions for one pass over BOTH images of an h x w pair."""
    return sum(2 * 2 * th * tw * c_out * c_in * k * k for (th, tw, _), (c_out, c_in, k) in zip(ops.lpips_tap_shapes(h, w), ops.LPIPS_CONVS))


def main():
    kernels_only = '--kernels' in sys.argv
    numbers = [int(a) for a in sys.argv[1:] if a.isdigit()]
    repeats = numbers[0] if numbers else (10 if kernels_only else 25)
    h, w = 756, 1008
    host_weights = lpips_reference.random_weights()
    gt_host, image_host, mask_host = lpips_reference.random_images(h, w)
    gt, image, mask = (torch.as_tensor(a).to(DEV) for a in (gt_host, image_host, mask_host))
    weights = qa.LpipsWeights(host_weights, DEV)
    for _ in range(3):
        ops.lpips_sums(gt, image, weights.packed, mask)
    torch.cuda.synchronize()
    if kernels_only:
        for _ in range(repeats):
            ops.lpips_sums(gt, image, weights.packed, mask)
        torch.cuda.synchronize()
        print(json.dumps({'what': 'kernel-trace pass', 'calls': repeats + 3}))
        return
    device_ms, call_ms = [], []
    for _ in range(repeats):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        ops.lpips_sums(gt, image, weights.packed, mask)
        stop.record()
        stop.synchronize()
        device_ms.append(start.elapsed_time(stop))
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = qa.lpips_metrics(image, gt, weights, mask)
        call_ms.append(1e3 * (time.perf_counter() - t0))
    host_ms = []
    for _ in range(3):
        t0 = time.perf_counter()
        want = lpips_reference.lpips(gt_host, image_host, host_weights, torch.float32)
        host_ms.append(1e3 * (time.perf_counter() - t0))
    assert abs(got['LPIPS'] - want['score']) < 5e-5, (got, want['score'])
    flops = conv_flops(h, w)
    median = statistics.median(device_ms)
    print(json.dumps({'what': 'LPIPS-alex of one 756x1008 pair: device_ms = one pass (ops.lpips_sums), call_ms = qa.lpips_metrics with a '
                              'mask (two passes)', 'repeats': repeats, 'device_ms_median': median, 'device_ms_min': min(device_ms),
                      'device_ms_max': max(device_ms), 'call_ms_median': statistics.median(call_ms),
                      'host_float32_restatement_ms_median': statistics.median(host_ms), 'host_threads': torch.get_num_threads(),
                      'conv_gflop_per_pass': flops / 1e9, 'conv_fraction_of_fp32_matrix_peak': flops / (median * 1e-3) / FP32_MATRIX_PEAK,
                      'LPIPS': got['LPIPS'], 'MaskedLPIPS': got['MaskedLPIPS']}))


if __name__ == '__main__':
    main()
