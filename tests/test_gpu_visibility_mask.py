"""Visibility masks on the device (csrc/visibility_mask.hip -> ops -> qa.visibility_mask -> harness.evaluate_frames) against the
fixtures the reference's MaskComputer / Warper produced (tests/golden/visibility_mask_*.npz) and, where there is no fixture, the
numpy restatement held to them (tests/mask_reference.py).  Both sides compute in fp64; the gates are those the fixtures were made
under: warping_mask equal on every pixel, warped_depth to 1e-12 relative (1e-8 where a training view equals the test view: a
coordinate that rounds across an integer moves a ~1e-13 weight to the neighbouring cell), masks equal on every pixel whose depth
error is not within 1e-9 x threshold of the threshold."""
import os

import numpy
import pytest
import torch

from tests import mask_reference

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
KEYS = ('extrinsics_train', 'extrinsic_test', 'intrinsics_train', 'intrinsic_test')


def dev(array):
    return torch.as_tensor(array).to(DEV)


def on_device(scene, views=slice(None), **kwargs):
    """qa.visibility_mask(return_views=True) on a scene dict -> the dict mask_reference.compare takes, as numpy."""
    from simplenerf_amd import qa
    mask, mask_views, warped_depth, weight_sum = qa.visibility_mask(
        dev(scene['depth_train'][views]), dev(scene['depth_test']), scene['extrinsics_train'][views], scene['extrinsic_test'],
        scene['intrinsics_train'][views], kwargs.pop('intrinsic_test', scene['intrinsic_test']), return_views=True, **kwargs)
    assert mask.dtype == torch.bool and mask_views.dtype == torch.bool and warped_depth.dtype == torch.float64
    assert mask.shape == scene['depth_test'].shape and mask_views.shape == scene['depth_train'][views].shape == weight_sum.shape
    out = {'mask': mask, 'mask_views': mask_views, 'warped_depth': warped_depth, 'weight_sum': weight_sum}
    out = {k: v.cpu().numpy() for k, v in out.items()}
    out['warping_mask'] = out['weight_sum'] > 0
    return out


def thresholds(scene, threshold=0.05):
    return [threshold * float(d.max()) for d in scene['depth_train']]


@pytest.mark.parametrize('shape', mask_reference.SHAPES)
@pytest.mark.parametrize('case', mask_reference.CASES)
def test_masks_equal_the_reference(case, shape):
    """Every fixture: per-view masks, the combined mask, warped_depth and warping_mask under the gates of the module docstring."""
    with numpy.load(os.path.join(GOLDEN, f'visibility_mask_{case}_{shape[0]}x{shape[1]}.npz')) as data:
        want = {k: data[k] for k in data.files}
    got = on_device(want, depth_error_threshold=float(want['depth_error_threshold']))
    figures = mask_reference.compare(got, want, want['depth_test'], want['thresholds'], 1e-8 if case == 'same_pose' else 1e-12)
    print(case, shape, figures)
    # the plain call returns the same mask, alone
    from simplenerf_amd import qa
    alone = qa.visibility_mask(dev(want['depth_train']), dev(want['depth_test']), *(want[k] for k in KEYS))
    assert isinstance(alone, torch.Tensor) and numpy.array_equal(alone.cpu().numpy(), got['mask'])


def test_min_views_counts_the_views():
    scene = mask_reference.occlusion_scene(37, 53, 'generic')
    three = on_device(scene)
    assert 0.05 < three['mask_views'].mean() < 0.95
    for v in range(3):          # T = 1 with min_views = 1: the single-view mask
        one = on_device(scene, slice(v, v + 1), min_views=1)
        assert numpy.array_equal(one['mask'], one['mask_views'][0]) and numpy.array_equal(one['mask'], three['mask_views'][v])
        assert numpy.array_equal(one['warped_depth'][0], three['warped_depth'][v])      # a view does not depend on its batch
    assert numpy.array_equal(on_device(scene, min_views=3)['mask'], three['mask_views'].all(0))
    assert numpy.array_equal(on_device(scene, min_views=1)['mask'], three['mask_views'].any(0))
    assert numpy.array_equal(three['mask'], three['mask_views'].sum(0) >= 2)


def test_two_calls_return_the_same_bits():
    scene = mask_reference.occlusion_scene(64, 80, 'behind')
    first, second = on_device(scene), on_device(scene)
    for key in ('mask', 'mask_views', 'warped_depth', 'weight_sum'):
        assert first[key].tobytes() == second[key].tobytes(), key


def test_a_frame_larger_than_a_tile_equals_the_restatement():
    """(96, 128), T = 3, no fixture: 144 workgroups of gather, 48 per view of project, a sort of 36 864 keys."""
    scene = mask_reference.occlusion_scene(96, 128, 'generic', seed=3)
    want = mask_reference.visibility_mask(scene['depth_train'], scene['depth_test'], *(scene[k] for k in KEYS))
    assert 0.05 < 1 - want['mask'].mean() < 0.6 and 0.05 < 1 - want['warping_mask'].mean() < 0.6
    got = on_device(scene)
    print(mask_reference.compare(got, want, scene['depth_test'], thresholds(scene), 1e-12))
    assert numpy.abs(got['weight_sum'] - want['weight_sum']).max() <= 1e-12 * want['weight_sum'].max()


def test_other_test_intrinsic_and_none():
    scene = mask_reference.occlusion_scene(37, 53, 'generic')
    other = scene['intrinsic_test'].copy()
    other[0, 0] *= 1.1
    other[1, 1] *= 0.95
    other[0, 2] += 1.5
    depth_test = mask_reference.ray_cast(scene['extrinsic_test'], other, 37, 53).astype(numpy.float32)
    scene = dict(scene, intrinsic_test=other, depth_test=depth_test)
    want = mask_reference.visibility_mask(scene['depth_train'], scene['depth_test'], *(scene[k] for k in KEYS))
    assert 0.3 < want['mask'].mean() < 0.95
    print(mask_reference.compare(on_device(scene), want, depth_test, thresholds(scene), 1e-12))
    # a missing test intrinsic: every training view's own -- here views with DIFFERENT intrinsics
    scene['intrinsics_train'] = numpy.stack([scene['intrinsics_train'][0], other, scene['intrinsics_train'][2]])
    scene['depth_train'] = numpy.stack([mask_reference.ray_cast(e, k, 37, 53) for e, k in
                                        zip(scene['extrinsics_train'], scene['intrinsics_train'])]).astype(numpy.float32)
    want = mask_reference.visibility_mask(scene['depth_train'], scene['depth_test'], scene['extrinsics_train'], scene['extrinsic_test'],
                                          scene['intrinsics_train'], None)
    got = on_device(scene, intrinsic_test=None)
    print(mask_reference.compare(got, want, depth_test, thresholds(scene), 1e-12))
    explicit = mask_reference.visibility_mask(scene['depth_train'], scene['depth_test'], *(scene[k] for k in KEYS))
    assert not numpy.array_equal(explicit['warped_depth'][0], want['warped_depth'][0])      # None is not "the given one"


def test_unpinned_sources_add_nothing():
    """A NaN / inf depth drops that source alone; a view of zero depth (max L = 0) drops the view: as the restatement does."""
    scene = mask_reference.occlusion_scene(24, 32, 'generic')
    depth = scene['depth_train'].copy()
    depth[0] = 0.0
    depth[1, 5, 7], depth[1, 6, 7], depth[2, 0, 0] = numpy.nan, numpy.inf, -numpy.inf
    scene = dict(scene, depth_train=depth)
    with numpy.errstate(invalid='ignore'):
        want = mask_reference.visibility_mask(scene['depth_train'], scene['depth_test'], *(scene[k] for k in KEYS))
    got = on_device(scene)
    assert not got['warping_mask'][0].any() and numpy.isfinite(got['warped_depth']).all()
    assert numpy.array_equal(got['warping_mask'], want['warping_mask']) and numpy.array_equal(got['mask_views'], want['mask_views'])
    scale = numpy.maximum(numpy.abs(want['warped_depth']), 1e-300)
    assert float((numpy.abs(got['warped_depth'] - want['warped_depth']) / scale).max()) <= 1e-12


def test_pose_conversion_is_consistent_on_the_synthetic_scene():
    """synth.extrinsic_of_pose: warping view 0's true depth into view 1 reproduces view 1's true depth on the warped pixels to
    within the depth threshold, on more than half of the frame.  The scene is one plane without occlusion, which allows a sharper
    bound than the threshold (0.2 here, which the inverse pose WITHOUT the axis flip also meets: its error is 0.14): a source that
    adds to a pixel lies less than one pixel from it in x and in y, and its Z is the plane's depth at its own position, so the
    warped depth is within gx + gy of the test depth, g the largest step of the test depth between neighbouring pixels (0.0012 +
    0.0052 for view 1); gated at 1.5 x that for the plane's curvature in depth.  Without the flip the error is above 0.1."""
    from simplenerf_amd import qa, synth
    scene = synth.synth_scene(0, 3, 48, 64)
    extrinsics = numpy.stack([synth.extrinsic_of_pose(p) for p in scene['poses']])
    intrinsics = scene['intrinsics'].astype(numpy.float64)
    for a, b in ((0, 1), (0, 2), (1, 2)):
        mask, views, warped, weights = qa.visibility_mask(dev(scene['true_depth'][a:a + 1]), dev(scene['true_depth'][b]), extrinsics[a:a + 1],
                                                          extrinsics[b], intrinsics[a:a + 1], intrinsics[b], min_views=1, return_views=True)
        landed = (weights[0] > 0).cpu().numpy()
        target = scene['true_depth'][b].astype(numpy.float64)
        error = numpy.abs(warped[0].cpu().numpy() - target)[landed]
        step = numpy.abs(numpy.diff(target, axis=1)).max() + numpy.abs(numpy.diff(target, axis=0)).max()
        print(a, b, 'warped', landed.mean(), 'largest depth error', error.max(), 'steps', step, 'threshold', 0.05 * scene['true_depth'][a].max())
        assert landed.mean() > 0.5 and error.max() < 0.05 * float(scene['true_depth'][a].max())
        assert error.max() <= 1.5 * step
        assert numpy.array_equal(mask.cpu().numpy(), landed) and mask.float().mean() > 0.5
    frames = synth.scene_mask_views(scene, 1)
    assert frames['depth_train'].shape == (2, 48, 64) and numpy.array_equal(frames['extrinsic_test'], extrinsics[1])
    assert numpy.array_equal(frames['extrinsics_train'], extrinsics[[0, 2]]) and frames['min_views'] == 2


def test_evaluate_frames_computes_the_mask_it_is_not_given():
    """A frame with 'mask_views' scores exactly as the same frame given the precomputed 'mask'; a frame with neither scores as before."""
    from simplenerf_amd import harness, qa
    from tests.test_gpu_qa import tiny_model_and_frames
    cfg, model, frames = tiny_model_and_frames('config1')
    plain = {k: v for k, v in frames[0].items() if k != 'mask'}
    assert 'mask' not in frames[0] and tuple(plain['camera']['resolution']) == (24, 32)
    scene = mask_reference.occlusion_scene(24, 32, 'generic')
    views = {k: scene[k] for k in ('depth_train', 'depth_test') + KEYS}
    mask = qa.visibility_mask(dev(scene['depth_train']), dev(scene['depth_test']), *(scene[k] for k in KEYS))
    assert 0.5 < float(mask.float().mean()) < 0.99
    device = torch.device(DEV)
    computed = harness.evaluate_frames(model, cfg, [dict(plain, mask_views=views)], device)
    given = harness.evaluate_frames(model, cfg, [dict(plain, mask=mask.cpu().numpy())], device)
    neither = harness.evaluate_frames(model, cfg, [plain], device)
    masked = ['MaskedRMSE', 'MaskedPSNR', 'MaskedSSIM', 'MaskedDepthRMSE', 'MaskedDepthMAE', 'MaskedDepthSROCC']
    row, want = computed['unrounded'][0], given['unrounded'][0]
    assert sorted(row) == sorted(want) and all(name in row for name in masked)
    assert all(numpy.float64(row[k]).tobytes() == numpy.float64(want[k]).tobytes() for k in row), (row, want)
    assert all(numpy.isfinite(row[name]) for name in masked)
    assert repr(computed) == repr(given)
    # a given mask wins over 'mask_views'; other thresholds reach the mask
    both = harness.evaluate_frames(model, cfg, [dict(plain, mask=numpy.ones((24, 32), dtype=bool), mask_views=views)], device)
    assert both['unrounded'][0]['MaskedRMSE'] == both['unrounded'][0]['RMSE'] != row['MaskedRMSE']
    strict = harness.evaluate_frames(model, cfg, [dict(plain, mask_views=dict(views, min_views=3, depth_error_threshold=0.01))], device)
    assert strict['unrounded'][0]['MaskedRMSE'] != row['MaskedRMSE']
    # neither: today's row
    old = neither['unrounded'][0]
    assert not any(k.startswith('Masked') for k in old) and sorted(old) == sorted(k for k in row if not k.startswith('Masked'))
    assert all(numpy.float64(old[k]).tobytes() == numpy.float64(row[k]).tobytes() for k in old)
    assert sorted(neither['average']) == sorted(k for k in old if k != 'frame_num')
