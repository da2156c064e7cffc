#!/usr/bin/env python3
"""Golden vectors for the visibility masks, made by RUNNING THE REFERENCE's classes here: ``MaskComputer.compute_mask`` and the
``Warper.forward_warp`` behind it (src/qa/00_Common/src/mask_generators), and the masked scripts' combination
``numpy.sum(masks, axis=0) > 1``.

    PYTHONDONTWRITEBYTECODE=1 python3 tools/make_golden_masks.py

Inputs are the analytic occlusion scene of tests/mask_reference.py (``occlusion_scene``: a slanted plane behind a sphere, three
training views, depths stored as float32) for every shape in ``SHAPES`` and every pose case in ``CASES``.  Each
``tests/golden/visibility_mask_<case>_<h>x<w>.npz`` stores the inputs, per training view the reference's ``warping_mask``,
``warped_depth`` and ``mask``, the per-view threshold, and the combined mask: data only.

The reference's threshold is ``0.05 * depth_train.max()`` with a float32 maximum, which numpy >= 2 evaluates in float32 and
numpy 1 in float64; this project takes the float64 product.  The generator asserts that no pixel's depth error lies between the
two, so the stored masks are those of either numpy.  It also asserts what the tests rely on: fragile pixels (a depth error within
1e-9 x threshold of the threshold) are at most 0.5 % of a case, the restatement of tests/mask_reference.py agrees with the
reference on every ``warping_mask`` pixel, 'behind' puts between 5 % and 50 % of the points behind the test camera with no |Z|
below 0.1, and an interior cell is only reached by sources whose unclipped floor cell lies in [0, h] x [0, w] -- the property the
device's inverted index is built on."""
import os
import sys
import types

import numpy

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = '/root/reference'
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REF, 'src', 'qa', '00_Common', 'src', 'mask_generators'))
for name in ('skimage', 'skimage.io', 'skimage.transform', 'simplejson', 'skvideo', 'skvideo.io'):
    sys.modules.setdefault(name, types.ModuleType(name))

from MaskComputer01 import MaskComputer  # noqa: E402  (the reference)

from tests import mask_reference  # noqa: E402

OUT = os.path.join(REPO, 'tests', 'golden')
THRESHOLD = 0.05


def reachable_only_from_keyed_cells(x, y, h, w):
    """Every source whose clipped corners include an interior cell has its unclipped floor cell in [0, h] x [0, w]."""
    fx, fy, cx, cy = numpy.floor(x), numpy.floor(y), numpy.ceil(x), numpy.ceil(y)
    inside = lambda v, n: (numpy.clip(v, 0, n + 1) >= 1) & (numpy.clip(v, 0, n + 1) <= n)
    reaches = (inside(fx, w) | inside(cx, w)) & (inside(fy, h) | inside(cy, h))
    keyed = (fx >= 0) & (fx <= w) & (fy >= 0) & (fy <= h)
    return bool(numpy.all(keyed[reaches]))


def run_case(case, h, w):
    scene = mask_reference.occlusion_scene(h, w, case)
    computer = MaskComputer({'depth_error_threshold': THRESHOLD})
    frame = numpy.zeros((h, w, 3), dtype=numpy.uint8)        # only feeds the warped image, which compute_mask discards
    arrays = dict(scene, depth_error_threshold=THRESHOLD)
    views = {'warping_mask': [], 'warped_depth': [], 'mask_views': [], 'thresholds': []}
    for v in range(3):
        args = (frame, scene['depth_train'][v], scene['depth_test'], scene['extrinsics_train'][v], scene['extrinsic_test'],
                scene['intrinsics_train'][v], scene['intrinsic_test'])
        mask = computer.compute_mask(*args)
        warping_mask, warped_depth = computer.warper.forward_warp(args[0], None, args[1], *args[3:])[1:3]
        threshold64 = THRESHOLD * float(scene['depth_train'][v].max())
        threshold32 = float(numpy.float32(THRESHOLD) * scene['depth_train'][v].max())
        error = numpy.abs(warped_depth - scene['depth_test'])
        lo, hi = min(threshold32, threshold64), max(threshold32, threshold64)
        assert not numpy.any(warping_mask & (error >= lo) & (error <= hi)), (case, h, w, v, 'a pixel between the two thresholds')
        assert numpy.array_equal(mask, warping_mask & (error < threshold64))
        assert warped_depth.dtype == numpy.float64 and mask.dtype == bool
        x, y, z = mask_reference.project(args[1], *args[3:])
        assert reachable_only_from_keyed_cells(x, y, h, w), (case, h, w, v)
        if case == 'behind':
            behind = float((z < 0).mean())
            assert 0.05 <= behind <= 0.5 and numpy.abs(z).min() >= 0.1, (h, w, v, behind, float(numpy.abs(z).min()))
        views['warping_mask'].append(warping_mask)
        views['warped_depth'].append(warped_depth)
        views['mask_views'].append(mask)
        views['thresholds'].append(threshold64)
    arrays.update({k: numpy.stack(a) for k, a in views.items()})
    arrays['mask'] = numpy.sum(arrays['mask_views'], axis=0) > 1
    own = mask_reference.visibility_mask(scene['depth_train'], scene['depth_test'], scene['extrinsics_train'], scene['extrinsic_test'],
                                         scene['intrinsics_train'], scene['intrinsic_test'], THRESHOLD)
    assert numpy.array_equal(own['warping_mask'], arrays['warping_mask']), (case, h, w)
    fragile = mask_reference.fragile(arrays['warped_depth'], scene['depth_test'], arrays['thresholds']) & arrays['warping_mask']
    assert fragile.mean() <= 0.005, (case, h, w, float(fragile.mean()))
    figures = mask_reference.compare(own, arrays, scene['depth_test'], arrays['thresholds'], 1e-8 if case == 'same_pose' else 1e-12)
    path = os.path.join(OUT, f'visibility_mask_{case}_{h}x{w}.npz')
    numpy.savez_compressed(path, **arrays)
    print(f'{os.path.basename(path)}: {os.path.getsize(path)} B; not visible {1 - arrays["mask"].mean():.3f}, holes '
          f'{1 - arrays["warping_mask"].mean():.3f}, fragile {int(fragile.sum())}; restatement: {figures}')


if __name__ == '__main__':
    for case_name in mask_reference.CASES:
        for height, width in mask_reference.SHAPES:
            run_case(case_name, height, width)
