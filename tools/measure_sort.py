#!/usr/bin/env python3
"""Time the HIP library's sorts and mask compaction (csrc/sort.hip) against the torch ops they can replace in the QA stage, at the
sizes of one 756 x 1008 frame.  A record, not a gate.
    python tools/measure_sort.py [repeats] [--only NAME]      -> one JSON line (--only: one pair, for a kernel trace of it alone)
Each figure: HIP events around what ONE call enqueues, warm (5 calls first), median of ``repeats`` (default 25), both sides in this
process, alternating.  The three pairs:
  sort_values            762 048 fp32 depths (the ground-truth depths of tools/measure_qa.py's frame)   | torch.sort(x).values
  sort_keys_with_order   the 2 286 144 splat keys of the frame with 3 training views, 22 bits            | torch.sort(keys, stable=True)
  compact_pair           two 762 048 fp32 arrays under a mask that keeps 70 %                            | a[keep], b[keep]
compact_pair and the boolean selections both end in a read of the kept count on the host, which the events include.  The results of
the two sides are compared for equality before anything is timed."""
import json
import os
import statistics
import sys

import numpy
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from simplenerf_amd import ops, qa  # noqa: E402
from tests import mask_reference  # noqa: E402

DEV = torch.device('cuda', 0)
KEYS = ('extrinsics_train', 'extrinsic_test', 'intrinsics_train', 'intrinsic_test')


def event_ms(call):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    call()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop)


def pair(name, library, vendor, repeats, extra):
    for _ in range(5):
        library()
        vendor()
    torch.cuda.synchronize()
    ours, theirs = [], []
    for _ in range(repeats):
        ours.append(event_ms(library))
        theirs.append(event_ms(vendor))
    out = {'library_ms_median': statistics.median(ours), 'library_ms_min': min(ours), 'library_ms_max': max(ours),
           'torch_ms_median': statistics.median(theirs), 'torch_ms_min': min(theirs), 'torch_ms_max': max(theirs)}
    out['library_over_torch'] = out['library_ms_median'] / out['torch_ms_median']
    out.update(extra)
    return name, out


def main():
    args = sys.argv[1:]
    only = args.pop(args.index('--only') + 1) if '--only' in args else None
    args = [a for a in args if a != '--only']
    repeats = int(args[0]) if args else 25
    h, w = 756, 1008
    rng = numpy.random.default_rng(0)
    y, x = numpy.mgrid[0:h, 0:w]
    gt_depth = (3 + numpy.sin(x / 40) + 0.5 * numpy.cos(y / 17) + rng.normal(0, 0.05, (h, w))).astype(numpy.float32)
    depth = numpy.maximum(gt_depth * 1.1 + rng.normal(0, 0.2, (h, w)) - 2.2, 0).astype(numpy.float32)
    g, e = torch.from_numpy(gt_depth).to(DEV).reshape(-1), torch.from_numpy(depth).to(DEV).reshape(-1)
    keep = torch.from_numpy(rng.random(h * w) < 0.7).to(DEV)
    scene = mask_reference.occlusion_scene(h, w, 'generic')
    cameras = torch.from_numpy(qa.visibility_cameras(*(scene[k] for k in KEYS))).to(DEV)
    keys = ops.visibility_mask_project(torch.as_tensor(scene['depth_train']).to(DEV), cameras)[1].reshape(-1)
    key_bits = (3 * ((h + 1) * (w + 1) + 1) - 1).bit_length()

    assert torch.equal(ops.sort_values(g).view(torch.int32), torch.sort(g).values.view(torch.int32))
    got_keys, got_order = ops.sort_keys_with_order(keys, key_bits)
    want_keys, want_order = torch.sort(keys, stable=True)
    assert torch.equal(got_keys, want_keys) and torch.equal(got_order, want_order)
    a, b = ops.compact_pair(g, e, keep)
    assert torch.equal(a, g[keep]) and torch.equal(b, e[keep])

    pairs = {
        'sort_values': (lambda: ops.sort_values(g), lambda: torch.sort(g).values, {'count': g.numel(), 'passes': 4}),
        'sort_keys_with_order': (lambda: ops.sort_keys_with_order(keys, key_bits), lambda: torch.sort(keys, stable=True),
                                 {'count': keys.numel(), 'key_bits': key_bits, 'passes': (key_bits + 7) // 8,
                                  'distinct_keys': int(torch.unique(keys).numel())}),
        'compact_pair': (lambda: ops.compact_pair(g, e, keep), lambda: (g[keep], e[keep]), {'count': g.numel(), 'kept': int(keep.sum())}),
    }
    if only is not None and only not in pairs:
        raise SystemExit(f'--only: expected one of {", ".join(pairs)}, got {only}')
    results = dict(pair(name, library, vendor, repeats, extra) for name, (library, vendor, extra) in pairs.items() if only in (None, name))
    print(json.dumps({'what': 'library sorts and mask compaction against the torch ops, sizes of one 756x1008 frame', 'repeats': repeats,
                      **results}))


if __name__ == '__main__':
    main()
