#!/usr/bin/env python3
"""Golden vectors for the Warper, made by RUNNING THE REFERENCE's class: ``Warper.forward_warp``, ``Warper.bilinear_splatting`` and
``Warper.bilinear_interpolation`` (src/qa/00_Common/src/mask_generators/Warper.py).

    PYTHONDONTWRITEBYTECODE=1 python3 tools/make_golden_warp.py --reference <checkout of the reference>

(or SIMPLENERF_REFERENCE in the environment).  Scenes are the analytic occlusion scene of tests/mask_reference.py for every shape in
``SHAPES`` and every pose case in ``CASES``; ``frame1`` is random uint8 from a fixed seed; ``mask1`` has about 10 % holes in
'generic' and 'behind' and is all-true in 'same_pose' (whose first view puts every source on an integer position up to rounding: a
hole there would leave cells to ~1e-13 weights alone).  Each ``tests/golden/warp_<case>_<h>x<w>.npz`` stores, data only:

  frame1 (3,h,w,3) uint8, mask1 (3,h,w) bool                      inputs beside the scene's (depths and matrices: occlusion_scene)
  warped_frame2, mask2, warped_depth2, flow12                      forward_warp of every training view
  colour_unrounded (3,h,w,3) float64                               bilinear_splatting of the float64 frame, is_image=False
  values4 (h,w,4) float64 >= 0, splat_flow_mask                    bilinear_splatting of values4 with depth_train[VIEW], flow12[VIEW],
  splat4, splat4_mask2                                             mask1[VIEW] and the random flow mask
  back_flow (h,w,2), back_flow_mask                                bilinear_interpolation along back_flow of: warped_frame2[VIEW] as an
  back_image, back_image_mask1, back_image_plain, ..._plain_mask1  image with (mask2[VIEW], back_flow_mask) and without masks, and of
  back_float, back_float_mask1, back_float_plain, ..._plain_mask1  warped_depth2[VIEW] (one channel) as a float frame, the same two ways

and asserts what the tests' gates rely on (below), failing instead of writing a file that breaks one."""
import argparse
import os
import sys
import types
import zipfile

import numpy

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
for name in ('skimage', 'skimage.io', 'skimage.transform', 'simplejson', 'skvideo', 'skvideo.io'):
    sys.modules.setdefault(name, types.ModuleType(name))

from tests import mask_reference, warp_reference  # noqa: E402

OUT = os.path.join(REPO, 'tests', 'golden')
LIMIT = 1 << 20            # bytes a committed file may have
VIEW = 1                   # the view whose flow the float splat and the backward warps use
HOLES = 0.1


def inputs(case, h, w):
    """The inputs that are not the scene's: one generator per file, drawn in a fixed order."""
    rng = numpy.random.RandomState(7000 + 1000 * h + w + 17 * mask_reference.CASES.index(case))
    frame1 = rng.randint(0, 256, (3, h, w, 3)).astype(numpy.uint8)
    holes = rng.random_sample((3, h, w)) < HOLES
    mask1 = numpy.ones((3, h, w), dtype=bool) if case == 'same_pose' else ~holes
    values4 = rng.randint(0, 1 << 16, (h, w, 4)) / 256.0             # non-negative, 16 significant bits: the file compresses
    splat_flow_mask = rng.random_sample((h, w)) >= HOLES
    back_flow_mask = rng.random_sample((h, w)) >= HOLES
    return {'frame1': frame1, 'mask1': mask1, 'values4': values4, 'splat_flow_mask': splat_flow_mask, 'back_flow_mask': back_flow_mask}


def light_weight_share(x, y, z, keep, h, w):
    """Largest share of a covered cell's weight that comes from contributions whose PROXIMITY weight is below 1e-6."""
    keep = keep & numpy.isfinite(x) & numpy.isfinite(y)
    log_depth = numpy.log(1.0 + numpy.clip(z, 0.0, 1000.0))
    divisor = numpy.exp(log_depth / log_depth.max() * 50.0)[keep]
    total, light = numpy.zeros((h + 2) * (w + 2)), numpy.zeros((h + 2) * (w + 2))
    for row, col, prox in warp_reference._corners(x[keep], y[keep], h, w):
        cell = (row * (w + 2) + col).astype(numpy.int64)
        total += numpy.bincount(cell, prox / divisor, minlength=total.size)
        light += numpy.bincount(cell, numpy.where(prox < 1e-6, prox, 0.0) / divisor, minlength=total.size)
    total, light = (a.reshape(h + 2, w + 2)[1:-1, 1:-1] for a in (total, light))
    covered = total > 0
    return float((light[covered] / total[covered]).max()) if covered.any() else 0.0


def save_npz(path, arrays):
    """numpy.savez_compressed with a fixed time stamp on every member: the same arrays give the same bytes on every run."""
    with zipfile.ZipFile(path, 'w') as archive:
        for key, value in arrays.items():
            info = zipfile.ZipInfo(key + '.npy', date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            with archive.open(info, 'w') as member:
                numpy.lib.format.write_array(member, numpy.asanyarray(value), allow_pickle=False)


def hold(got, want, what, exact=False):
    """The restatement against the reference: masks equal, float outputs within 1e-12 relative (or bit-equal)."""
    got, want = numpy.asarray(got), numpy.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if exact or got.dtype != numpy.float64:
        assert got.tobytes() == want.tobytes(), (what, 'differs')
        return 0.0
    worst = warp_reference.relative(got, want)
    assert worst <= 1e-12, (what, worst)
    return worst


def run_case(warper, case, h, w):
    scene = mask_reference.occlusion_scene(h, w, case)
    arrays = inputs(case, h, w)
    views = {'warped_frame2': [], 'mask2': [], 'warped_depth2': [], 'flow12': [], 'colour_unrounded': []}
    figures = {'ties': 0.0, 'light': 0.0, 'min_abs_z': numpy.inf, 'restatement': 0.0}
    for v in range(3):
        camera = (scene['extrinsics_train'][v], scene['extrinsic_test'], scene['intrinsics_train'][v], scene['intrinsic_test'])
        frame1, mask1, depth1 = arrays['frame1'][v], arrays['mask1'][v], scene['depth_train'][v]
        warped_frame2, mask2, warped_depth2, flow12 = warper.forward_warp(frame1, mask1, depth1, *camera)
        z = warper.compute_transformed_points(depth1, *camera)[:, :, 2, 0]
        unrounded, unrounded_mask = warper.bilinear_splatting(frame1.astype(numpy.float64), mask1, z, flow12, None, is_image=False)
        assert warped_frame2.dtype == numpy.uint8 and mask2.dtype == bool and warped_depth2.dtype == flow12.dtype == numpy.float64
        assert numpy.array_equal(unrounded_mask, mask2)
        assert numpy.array_equal(numpy.round(numpy.clip(unrounded, 0, 255)).astype(numpy.uint8), warped_frame2)
        # ---- the conditions the gates rely on
        x, y = warp_reference.positions(flow12)
        on_integer = (numpy.abs(x - numpy.round(x)) <= 1e-9) | (numpy.abs(y - numpy.round(y)) <= 1e-9)
        if case != 'same_pose':
            assert not on_integer.any(), (case, h, w, v, int(on_integer.sum()), 'sources within 1e-9 of an integer position')
        light = light_weight_share(x, y, z, mask1, h, w)
        assert light <= 1e-6, (case, h, w, v, light, 'a covered cell takes more than 1e-6 of its weight from proximity weights < 1e-6')
        assert numpy.abs(z).min() > 0.1, (case, h, w, v, float(numpy.abs(z).min()))
        ties = float(warp_reference.near_tie(unrounded)[mask2].mean()) if mask2.any() else 0.0
        assert ties <= 1e-3, (case, h, w, v, ties, 'unrounded colour values within 1e-9 of a rounding tie')
        # ---- the restatement against the reference
        own = warp_reference.forward_warp(frame1, depth1, *camera, mask1=mask1)
        hold(own[1], mask2, 'mask2')
        worst = hold(own[2], warped_depth2, 'warped_depth2')      # (1e-12 in every case, same_pose included: both sides are numpy)
        deviation = warp_reference.flow_deviation(own[3], flow12)
        assert deviation <= 1e-12, (case, h, w, v, 'flow12', deviation)
        own_unrounded = warp_reference.bilinear_splatting(frame1.astype(numpy.float64), z, flow12, mask1)[0]
        worst = max(worst, hold(own_unrounded, unrounded, 'colour_unrounded'))
        wrong, inside = warp_reference.colour_difference(own[0], warped_frame2, unrounded)
        assert wrong == 0 and inside <= 1, (case, h, w, v, 'warped_frame2', wrong, inside)
        figures = {'ties': max(figures['ties'], ties), 'light': max(figures['light'], light),
                   'min_abs_z': min(figures['min_abs_z'], float(numpy.abs(z).min())), 'restatement': max(figures['restatement'], worst)}
        for key, value in zip(views, (warped_frame2, mask2, warped_depth2, flow12, unrounded)):
            views[key].append(value)
    arrays.update({k: numpy.stack(a) for k, a in views.items()})
    # ---- a float frame of four channels along the stored flow, with a source mask and a flow mask
    # (the depth widened first: handed a float32 depth1 the reference would compute its depth weights in float32; this project's
    # arithmetic is fp64 on inputs widened first, as forward_warp's own transformed depth is)
    splat_args = (arrays['mask1'][VIEW], scene['depth_train'][VIEW].astype(numpy.float64), arrays['flow12'][VIEW], arrays['splat_flow_mask'])
    arrays['splat4'], arrays['splat4_mask2'] = warper.bilinear_splatting(arrays['values4'], *splat_args, is_image=False)
    x, y = warp_reference.positions(arrays['flow12'][VIEW])
    light = light_weight_share(x, y, splat_args[1], splat_args[0] & splat_args[3], h, w)
    assert light <= 1e-6 and arrays['values4'].min() >= 0, (case, h, w, light)
    own = warp_reference.bilinear_splatting(arrays['values4'], splat_args[1], splat_args[2], splat_args[0], splat_args[3])
    hold(own[1], arrays['splat4_mask2'], 'splat4_mask2')
    figures['restatement'] = max(figures['restatement'], hold(own[0], arrays['splat4'], 'splat4'))
    # ---- the backward warp: along the flow of another view, so that positions fall between pixels and off the frame
    arrays['back_flow'] = arrays['flow12'][2]
    image, known, depth = arrays['warped_frame2'][VIEW], arrays['mask2'][VIEW], arrays['warped_depth2'][VIEW][..., None]
    for name, frame, is_image in (('back_image', image, True), ('back_float', depth, False)):
        for suffix, masks in (('', (known, arrays['back_flow'], arrays['back_flow_mask'])), ('_plain', (None, arrays['back_flow'], None))):
            warped, mask1 = warper.bilinear_interpolation(frame, *masks, is_image=is_image)
            arrays[name + suffix], arrays[name + suffix + '_mask1'] = warped, mask1
            own = warp_reference.bilinear_interpolation(frame, masks[1], masks[0], masks[2], is_image=is_image)
            hold(own[0], warped, name + suffix, exact=True)
            hold(own[1], mask1, name + suffix + '_mask1', exact=True)
            assert 0.05 < mask1.mean() <= 1.0, (case, h, w, name + suffix, float(mask1.mean()))
    path = os.path.join(OUT, f'warp_{case}_{h}x{w}.npz')
    save_npz(path, arrays)
    size = os.path.getsize(path)
    assert size < LIMIT, (path, size)
    print(f'{os.path.basename(path)}: {size} B; landed {arrays["mask2"].mean():.3f}, ties {figures["ties"]:.2e}, light weight share '
          f'{figures["light"]:.2e}, min |Z| {figures["min_abs_z"]:.3f}, restatement {figures["restatement"]:.2e}')


if __name__ == '__main__':
    parser = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    parser.add_argument('--reference', default=os.environ.get('SIMPLENERF_REFERENCE'), help='a checkout of the reference project')
    root = parser.parse_args().reference
    if not root or not os.path.isdir(os.path.join(root, 'src', 'qa', '00_Common', 'src', 'mask_generators')):
        sys.exit('make_golden_warp: --reference (or SIMPLENERF_REFERENCE) must name a checkout of the reference project')
    sys.path.insert(0, os.path.join(root, 'src', 'qa', '00_Common', 'src', 'mask_generators'))
    from Warper import Warper  # noqa: E402  (the reference)
    for case_name in mask_reference.CASES:
        for height, width in mask_reference.SHAPES:
            run_case(Warper(), case_name, height, width)
