#!/usr/bin/env python3
"""Time LPIPS of ONE 756 x 1008 frame pair with a mask (LPIPS + MaskedLPIPS: two passes of the network over two images each) on the
device, and the float32 torch restatement the tests use (tests/lpips_reference.py) on the same box's CPU threads.  A record, not a
gate.  Random weights (lpips_reference.random_weights): the arithmetic does not depend on their values.
    python tools/measure_lpips.py [repeats]          -> one JSON line
    python tools/measure_lpips.py --kernels [calls]  -> only `calls` (default 10) warm ops.lpips_sums calls, for a run under
                                                        rocprofv3 --kernel-trace --stats (the per-kernel times; every convolution
                                                        geometry is its own instantiation conv_relu_kernel<k, s, p, c_in, c_out>)
    python tools/measure_lpips.py --net vgg ...      -> the same for the VGG-16 backbone (default: alex); --out FILE also writes
                                                        the JSON record there (profiles/)
device_ms: HIP events around what ONE ``ops.lpips_sums`` enqueues (prepare, five convolutions, two pools, five layer reductions,
the fold), warm, median of ``repeats`` (default 25); call_ms: a host clock around ``qa.lpips_metrics`` with the mask (two such
passes and the copy of ten scalars to the host); host_ms: the float32 restatement of one pass, median of 3.
conv_fraction_of_fp32_matrix_peak counts 2 x 10.8 GMAC = 43.4 GFLOP per pass (VGG-16: 2 x 233 GMAC = 0.93 TFLOP) against device_ms
(an upper bound on the convolutions' time: the other kernels are inside it) and the MI355X's 157.3 TFLOP/s fp32 matrix peak."""
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from simplenerf_amd import ops, qa  # noqa: E402
from tests import lpips_reference, lpips_vgg_reference  # noqa: E402

DEV = torch.device('cuda', 0)
FP32_MATRIX_PEAK = 157.3e12


def conv_flops(h, w, net='alex'):
    """2 x multiply-accumulates of the network's convolutions for one pass over BOTH images of an h x w pair."""
    if net == 'alex':
        return sum(2 * 2 * th * tw * c_out * c_in * k * k for (th, tw, _), (c_out, c_in, k) in zip(ops.lpips_tap_shapes(h, w), ops.LPIPS_CONVS))
    taps = ops.lpips_tap_shapes(h, w, net)
    total, tap = 0, 0
    for l, (c_out, c_in, k) in enumerate(ops.LPIPS_VGG_CONVS):          # a convolution has the extent of the tap that follows it
        th, tw, _ = taps[tap]
        total += 2 * 2 * th * tw * c_out * c_in * k * k
        tap += l in ops.LPIPS_VGG_TAP_CONVS
    return total


def main():
    kernels_only = '--kernels' in sys.argv
    arguments = sys.argv[1:]
    net = arguments[arguments.index('--net') + 1] if '--net' in arguments else 'alex'
    out = arguments[arguments.index('--out') + 1] if '--out' in arguments else None
    numbers = [int(a) for a in arguments if a.isdigit()]
    repeats = numbers[0] if numbers else (10 if kernels_only else 25)
    h, w = 756, 1008
    reference = lpips_vgg_reference if net == 'vgg' else lpips_reference
    host_weights = reference.random_weights()
    gt_host, image_host, mask_host = lpips_reference.random_images(h, w)
    gt, image, mask = (torch.as_tensor(a).to(DEV) for a in (gt_host, image_host, mask_host))
    weights = qa.LpipsWeights(host_weights, DEV, net=net)
    for _ in range(3):
        ops.lpips_sums(gt, image, weights.packed, mask, net=net)
    torch.cuda.synchronize()
    if kernels_only:
        for _ in range(repeats):
            ops.lpips_sums(gt, image, weights.packed, mask, net=net)
        torch.cuda.synchronize()
        print(json.dumps({'what': 'kernel-trace pass', 'net': net, 'calls': repeats + 3}))
        return
    device_ms, call_ms = [], []
    for _ in range(repeats):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        ops.lpips_sums(gt, image, weights.packed, mask, net=net)
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
        want = reference.lpips(gt_host, image_host, host_weights, torch.float32)
        host_ms.append(1e3 * (time.perf_counter() - t0))
    assert abs(got['LPIPS'] - want['score']) < 5e-5, (got, want['score'])
    flops = conv_flops(h, w, net)
    median = statistics.median(device_ms)
    record = json.dumps({'what': f'LPIPS-{net} of one 756x1008 pair: device_ms = one pass (ops.lpips_sums), call_ms = qa.lpips_metrics with a '
                                 'mask (two passes)', 'repeats': repeats, 'device_ms_median': median, 'device_ms_min': min(device_ms),
                         'device_ms_max': max(device_ms), 'call_ms_median': statistics.median(call_ms),
                         'host_float32_restatement_ms_median': statistics.median(host_ms), 'host_threads': torch.get_num_threads(),
                         'conv_gflop_per_pass': flops / 1e9, 'conv_fraction_of_fp32_matrix_peak': flops / (median * 1e-3) / FP32_MATRIX_PEAK,
                         'LPIPS': got['LPIPS'], 'MaskedLPIPS': got['MaskedLPIPS']})
    print(record)
    if out:
        with open(out, 'w') as f:
            f.write(record + '\n')


if __name__ == '__main__':
    main()
