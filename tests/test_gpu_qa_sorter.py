"""``sorter='library'`` (the HIP library's radix sort and compaction, csrc/sort.hip) against the default ``sorter='torch'`` in
qa.depth_metrics, qa.visibility_mask and harness.evaluate_frames.  A sorted array is unique and so is the stable order of a sort, so
the two sorters must give the same values: every comparison is ``==`` (NaN with NaN), none has a tolerance."""
import glob
import math
import os

import numpy
import pytest
import torch

from simplenerf_amd import qa

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
MASK_CASES = sorted(os.path.basename(p) for p in glob.glob(os.path.join(GOLDEN, 'visibility_mask_*.npz')))


def same(a: float, b: float) -> bool:
    return a == b or (math.isnan(a) and math.isnan(b))


@pytest.mark.parametrize('shape', [(24, 32), (37, 53), (64, 80)])
def test_depth_metrics_do_not_depend_on_the_sorter(shape):
    """Depths quantised to 1/8 (ties are plentiful); no mask, a random mask, an all-false mask."""
    h, w = shape
    rng = numpy.random.default_rng(h * 100 + w)
    gt = numpy.round((2.0 + rng.random((h, w)) * 6.0) * 8) / 8
    noisy = numpy.round((gt + rng.standard_normal((h, w)) * 0.5) * 8) / 8
    assert len(numpy.unique(gt)) < h * w / 4 and len(numpy.unique(noisy)) < h * w / 2
    gt_dev, eval_dev = (torch.from_numpy(v.astype(numpy.float32)).to(DEV) for v in (gt, noisy))
    masks = {'none': None, 'random': torch.from_numpy(rng.random((h, w)) < 0.6).to(DEV),
             'bytes': torch.from_numpy((rng.random((h, w)) < 0.3).astype(numpy.uint8) * 255).to(DEV),
             'all_false': torch.zeros((h, w), dtype=torch.bool, device=DEV)}
    for name, mask in masks.items():
        want = qa.depth_metrics(eval_dev, gt_dev, 0.5, 2.0, mask)
        got = qa.depth_metrics(eval_dev, gt_dev, 0.5, 2.0, mask, sorter='library')
        assert sorted(got) == sorted(want) and len(want) == (3 if mask is None else 6)
        assert all(same(got[k], want[k]) for k in want), (name, got, want)
        assert all(math.isfinite(v) for v in want.values()) == (name != 'all_false'), (name, want)
        assert same(want['DepthSROCC'], qa.depth_metrics(eval_dev, gt_dev, 0.5, 2.0, mask, sorter='torch')['DepthSROCC'])
    assert math.isnan(got['MaskedDepthSROCC']) and math.isnan(got['MaskedDepthRMSE'])       # (all_false is the last one)


@pytest.mark.parametrize('case', MASK_CASES)
def test_visibility_masks_do_not_depend_on_the_sorter(case):
    """Every committed fixture: mask, per-view masks, warped depths and weight sums equal between the two sorters."""
    assert len(MASK_CASES) >= 9
    with numpy.load(os.path.join(GOLDEN, case)) as data:
        scene = {k: data[k] for k in data.files}
    args = (torch.from_numpy(scene['depth_train']).to(DEV), torch.from_numpy(scene['depth_test']).to(DEV), scene['extrinsics_train'],
            scene['extrinsic_test'], scene['intrinsics_train'], scene['intrinsic_test'])
    threshold = float(scene['depth_error_threshold'])
    want = qa.visibility_mask(*args, depth_error_threshold=threshold, return_views=True)
    got = qa.visibility_mask(*args, depth_error_threshold=threshold, return_views=True, sorter='library')
    assert len(got) == len(want) == 4
    for a, b in zip(got, want):
        assert a.dtype == b.dtype and torch.equal(a, b)
    alone = qa.visibility_mask(*args, depth_error_threshold=threshold, sorter='library')
    assert isinstance(alone, torch.Tensor) and torch.equal(alone, want[0])


def test_evaluate_frames_passes_the_sorter_through():
    """A frame with a depth target and 'mask_views': the rows of the two sorters are the same bits."""
    from simplenerf_amd import harness
    from tests import mask_reference
    from tests.test_gpu_qa import tiny_model_and_frames
    cfg, model, frames = tiny_model_and_frames('config1')
    scene = mask_reference.occlusion_scene(24, 32, 'generic')
    keys = ('depth_train', 'depth_test', 'extrinsics_train', 'extrinsic_test', 'intrinsics_train', 'intrinsic_test')
    frame = dict({k: v for k, v in frames[0].items() if k != 'mask'}, mask_views={k: scene[k] for k in keys})
    assert frame.get('depth') is not None
    device = torch.device(DEV)
    want = harness.evaluate_frames(model, cfg, [frame], device)
    got = harness.evaluate_frames(model, cfg, [frame], device, sorter='library')
    row = want['unrounded'][0]
    assert 'MaskedDepthSROCC' in row and 'DepthMAE' in row and math.isfinite(row['MaskedDepthSROCC'])
    assert all(same(got['unrounded'][0][k], row[k]) for k in row) and repr(got) == repr(want)
