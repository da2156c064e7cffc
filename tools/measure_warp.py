#!/usr/bin/env python3
"""Time the Warper on ONE 756 x 1008 frame on the device -- every stage and the whole of ``qa.forward_warp``, and
``qa.bilinear_interpolation`` -- and with the host restatement the tests use (tests/warp_reference.py: numpy) on the same box.  A
record, not a gate.
    python tools/measure_warp.py [repeats] [--sorter torch|library]      -> one JSON line
stage_ms / device_ms: HIP events around what the stage / the whole call enqueues (project + the fold of its maxima, the stable sort
of the keys -- torch's or, with ``--sorter library``, the HIP library's -- the list starts, the colour gather, the depth gather),
warm, median of ``repeats`` (default 25); call_ms: a host clock around the call, matrices inverted on the host and copied, to the
synchronised result; host_ms: the restatement, median of 3.  The scene is the analytic occlusion scene of the fixtures (a sphere in
front of a slanted plane) at that resolution, view 1 warped into the test view with about 10 % of the source mask false; the backward
warp pulls the warped colour back along another view's flow.  The deviations are REPORTED: the 1e-12 gates of the tests belong to
their shapes (a position near 1000 carries a few ulps, which a small proximity weight at an occlusion edge amplifies)."""
import json
import os
import statistics
import sys
import time

import numpy
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from simplenerf_amd import ops, qa  # noqa: E402
from tests import mask_reference, warp_reference  # noqa: E402

DEV = torch.device('cuda', 0)
H, W, VIEW = 756, 1008, 1


def timed(stages, name, call):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    out = call()
    stop.record()
    stages.setdefault(name, []).append((start, stop))
    return out


def enqueue(frame1, depth1, camera, mask1, stages, sorter):
    """What qa.forward_warp puts on the stream, stage by stage."""
    h, w = depth1.shape
    points, keys, stats, flow12 = timed(stages, 'project', lambda: ops.warp_project(depth1, camera, mask1))
    if sorter == 'library':
        key_bits = ((h + 1) * (w + 1)).bit_length()
        sorted_keys, order = timed(stages, 'sort', lambda: ops.sort_keys_with_order(keys.reshape(-1), key_bits))
    else:
        sorted_keys, order = timed(stages, 'sort', lambda: torch.sort(keys.reshape(-1), stable=True))
    starts = timed(stages, 'list_starts', lambda: ops.visibility_mask_list_starts(sorted_keys, 1, h, w))
    colour = timed(stages, 'gather_colour', lambda: ops.warp_splat_gather(points, order, starts, stats, frame1, is_image=True))
    depth = timed(stages, 'gather_depth', lambda: ops.warp_splat_gather(points, order, starts, stats, points[0, 2].unsqueeze(-1)))
    return colour, depth, flow12


def medians(stages):
    return {name: statistics.median(a.elapsed_time(b) for a, b in events) for name, events in stages.items()}


def host_clock(call, repeats):
    out = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        result = call()
        torch.cuda.synchronize()
        out.append(1e3 * (time.perf_counter() - t0))
    return statistics.median(out), result


def main():
    args = sys.argv[1:]
    sorter = args.pop(args.index('--sorter') + 1) if '--sorter' in args else 'torch'
    args = [a for a in args if a != '--sorter']
    qa._sorter(sorter)
    repeats = int(args[0]) if args else 25
    scene = mask_reference.occlusion_scene(H, W, 'generic')
    rng = numpy.random.RandomState(1)
    frame1 = rng.randint(0, 256, (H, W, 3)).astype(numpy.uint8)
    mask1 = rng.random_sample((H, W)) >= 0.1
    matrices = (scene['extrinsics_train'][VIEW], scene['extrinsic_test'], scene['intrinsics_train'][VIEW], scene['intrinsic_test'])
    on_device = [torch.as_tensor(a).to(DEV) for a in (frame1, scene['depth_train'][VIEW], mask1)]
    camera = torch.from_numpy(qa.visibility_cameras(matrices[0][None], matrices[1], matrices[2][None], matrices[3])[0]).to(DEV)
    forward = lambda: qa.forward_warp(on_device[0], on_device[1], *matrices, mask1=on_device[2], sorter=sorter)
    for _ in range(5):
        enqueue(on_device[0], on_device[1], camera, on_device[2], {}, sorter)
    torch.cuda.synchronize()
    stages = {}
    for _ in range(repeats):
        timed(stages, 'whole', lambda: enqueue(on_device[0], on_device[1], camera, on_device[2], stages, sorter))
    torch.cuda.synchronize()
    stage_ms = medians(stages)
    whole = [a.elapsed_time(b) for a, b in stages['whole']]
    del stage_ms['whole']
    call_ms, got = host_clock(forward, repeats)
    colour, mask2, depth2, flow12 = (t.cpu().numpy() for t in got)
    # the backward warp: the warped colour pulled back along another view's flow, with both masks
    back_flow = warp_reference.flow_of(scene['depth_train'][2], scene['extrinsics_train'][2], *matrices[1:])[0]
    back_mask = rng.random_sample((H, W)) >= 0.1
    back_args = [got[0], torch.as_tensor(back_flow).to(DEV), got[1], torch.as_tensor(back_mask).to(DEV)]
    backward = lambda: qa.bilinear_interpolation(*back_args, is_image=True)
    backward_float = lambda: qa.bilinear_interpolation(got[2].unsqueeze(-1), *back_args[1:])
    for _ in range(5):
        backward()
    torch.cuda.synchronize()
    back_stages = {}
    for _ in range(repeats):
        timed(back_stages, 'interpolate_image', backward)
        timed(back_stages, 'interpolate_float', backward_float)
    torch.cuda.synchronize()
    back_call_ms, back_got = host_clock(backward, repeats)
    back_float_got = backward_float()
    # ---- the host restatement, and the deviations from it
    host_ms, back_host_ms = [], []
    for _ in range(3):
        t0 = time.perf_counter()
        want = warp_reference.forward_warp(frame1, scene['depth_train'][VIEW], *matrices, mask1=mask1)
        host_ms.append(1e3 * (time.perf_counter() - t0))
        t0 = time.perf_counter()
        want_back = warp_reference.bilinear_interpolation(colour, back_flow, mask2, back_mask, is_image=True)
        back_host_ms.append(1e3 * (time.perf_counter() - t0))
    want_back_float = warp_reference.bilinear_interpolation(depth2[..., None], back_flow, mask2, back_mask)
    unrounded = warp_reference.bilinear_splatting(frame1, warp_reference.flow_of(scene['depth_train'][VIEW], *matrices)[1], want[3], mask1)[0]
    wrong, inside = warp_reference.colour_difference(colour, want[0], unrounded)
    figures = {'mask2_differing': int((mask2 != want[1]).sum()), 'warped_depth2_relative': warp_reference.relative(depth2, want[2], want[1] & mask2),
               'flow12_deviation': warp_reference.flow_deviation(flow12, want[3]), 'colour_differing_outside_tie_band': wrong,
               'colour_largest_difference_in_tie_band': inside, 'colour_differing': int((colour != want[0]).sum()),
               'interpolate_image_equal': bool(numpy.array_equal(back_got[0].cpu().numpy(), want_back[0])),
               'interpolate_float_bit_equal': back_float_got[0].cpu().numpy().tobytes() == want_back_float[0].tobytes(),
               'interpolate_masks_equal': bool(numpy.array_equal(back_got[1].cpu().numpy(), want_back[1]))}
    print(json.dumps({'what': 'forward_warp and bilinear_interpolation of one 756x1008 frame', 'repeats': repeats, 'sorter': sorter,
                      'forward_warp': {'device_ms_median': statistics.median(whole), 'device_ms_min': min(whole), 'device_ms_max': max(whole),
                                       'stage_ms_median': stage_ms, 'call_ms_median': call_ms,
                                       'host_restatement_ms_median': statistics.median(host_ms), 'landed': float(mask2.mean())},
                      'bilinear_interpolation': {'device_ms_median': medians(back_stages), 'call_ms_median': back_call_ms,
                                                 'host_restatement_ms_median': statistics.median(back_host_ms),
                                                 'known': float(back_got[1].float().mean())},
                      'host_threads': torch.get_num_threads(), 'against_restatement': figures}))


if __name__ == '__main__':
    main()
