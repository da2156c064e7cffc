"""LPIPS on the device (csrc/lpips.hip -> ops.lpips_sums -> qa.lpips_metrics -> harness.evaluate_frames) against the float64
restatement of the package's definition (tests/lpips_reference.py).

Tolerances.  The reference computes LPIPS in float32, so its precision class is the distance of the float32 restatement from the
float64 one over the four test shapes with the seeded inputs of lpips_reference (measured by lpips_reference.precision_class on the
CPU; tests/test_lpips_host.py measures it again and compares with the figures committed here):
  * FEATURE_MEASURED = 7.49e-7   max over shapes and taps of max|x32 - x64| / max|x64|; the gate is 4 x that: another, equally valid
    order of the k sum on the matrix cores against the CPU's blocked convolution -- it does not admit a 16-bit operand (2^-9);
  * SUM_MEASURED = 1.65e-6       max over shapes and layers of |s32 - s64| / |s64|; the gate is 8 x that: one scalar's deviation is a
    noisier sample than a maximum over thousands of elements;
  * the score is also within 5e-5 absolute, half a unit of the 4th decimal the reference's scripts round to.
Reached on an MI355X: DESIGN.md, "LPIPS"."""
import functools

import numpy
import pytest
import torch

from tests import lpips_reference

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
FEATURE_MEASURED = 7.493379857719179e-07
SUM_MEASURED = 1.6480594426719216e-06
FEATURE_TOLERANCE = 4 * FEATURE_MEASURED
SUM_TOLERANCE = 8 * SUM_MEASURED
SCORE_CAP = 5e-5
SHAPES = lpips_reference.SHAPES


def dev(array):
    return torch.as_tensor(array).to(DEV)


@functools.lru_cache(maxsize=None)
def host_weights():
    return lpips_reference.random_weights()


@functools.lru_cache(maxsize=None)
def device_weights():
    from simplenerf_amd import qa
    return qa.LpipsWeights(host_weights(), DEV)


@functools.lru_cache(maxsize=None)
def case(shape):
    """The seeded pair and mask of a shape with the float64 restatement's results, plain and masked: computed once, never written."""
    gt, image, mask = lpips_reference.random_images(*shape)
    return {'gt': gt, 'image': image, 'mask': mask, 'plain': lpips_reference.lpips(gt, image, host_weights()),
            'masked': lpips_reference.lpips(gt, image, host_weights(), mask=mask)}


def score_of(sums, shape):
    from simplenerf_amd import ops
    return float(sum(numpy.float64(s) / (th * tw) for s, (th, tw, _) in zip(sums, ops.lpips_tap_shapes(*shape))))


@pytest.mark.parametrize('shape', SHAPES)
def test_taps_equal_the_restatement(shape):
    """Every post-ReLU tap of both images: a wrong pad, stride, tail or tap order shows here."""
    from simplenerf_amd import ops
    c = case(shape)
    _, taps = ops.lpips_sums(dev(c['gt']), dev(c['image']), device_weights().packed, return_taps=True)
    assert [tuple(t.shape) for t in taps] == [(2, th, tw, ch) for th, tw, ch in ops.lpips_tap_shapes(*shape)]
    for layer, (got, want) in enumerate(zip(taps, c['plain']['taps'])):
        got = got.permute(0, 3, 1, 2).double().cpu()
        assert got.shape == want.shape
        worst = float((got - want).abs().max() / want.abs().max())
        print(shape, 'tap', layer, tuple(want.shape), 'max|x - x64| / max|x64| =', worst, 'active', float((want > 0).double().mean()))
        assert worst <= FEATURE_TOLERANCE


@pytest.mark.parametrize('shape', SHAPES)
def test_sums_and_score_equal_the_restatement(shape):
    from simplenerf_amd import ops, qa
    c = case(shape)
    for name, mask in (('plain', None), ('masked', c['mask'])):
        want = c[name]
        assert 0.005 < want['score'] < 0.05                   # nothing degenerates
        sums = ops.lpips_sums(dev(c['gt']), dev(c['image']), device_weights().packed, None if mask is None else dev(mask)).cpu().numpy()
        deviations = [abs(g - w) / abs(w) for g, w in zip(sums, want['sums'])]
        score = score_of(sums, shape)
        print(shape, name, 'layer sums relative', deviations, 'score', score, 'want', want['score'], 'off', abs(score - want['score']))
        assert max(deviations) <= SUM_TOLERANCE
        assert abs(score - want['score']) <= min(SUM_TOLERANCE * want['score'], SCORE_CAP)
    metrics = qa.lpips_metrics(dev(c['image']), dev(c['gt']), device_weights(), dev(c['mask']))
    assert sorted(metrics) == ['LPIPS', 'MaskedLPIPS']
    assert abs(metrics['LPIPS'] - c['plain']['score']) <= min(SUM_TOLERANCE * c['plain']['score'], SCORE_CAP)
    assert abs(metrics['MaskedLPIPS'] - c['masked']['score']) <= min(SUM_TOLERANCE * c['masked']['score'], SCORE_CAP)
    assert sorted(qa.lpips_metrics(dev(c['image']), dev(c['gt']), device_weights())) == ['LPIPS']


@pytest.mark.parametrize('shape', SHAPES)
def test_exact_properties(shape):
    """All-true mask = the plain score bit for bit; all-false mask and identical images = 0.0 exactly; the two argument orders and
    two calls return the same bits."""
    from simplenerf_amd import ops, qa
    c = case(shape)
    gt, image, weights = dev(c['gt']), dev(c['image']), device_weights()
    plain = ops.lpips_sums(gt, image, weights.packed).cpu().numpy()
    assert numpy.all(plain > 0)
    assert numpy.array_equal(plain, ops.lpips_sums(gt, image, weights.packed).cpu().numpy())
    assert numpy.array_equal(plain, ops.lpips_sums(image, gt, weights.packed).cpu().numpy())
    assert numpy.array_equal(plain, ops.lpips_sums(gt, image, weights.packed, torch.ones(shape, dtype=torch.bool, device=DEV)).cpu().numpy())
    assert numpy.array_equal(plain, ops.lpips_sums(gt, image, weights.packed, torch.ones(shape, dtype=torch.uint8, device=DEV)).cpu().numpy())
    none = torch.zeros(shape, dtype=torch.bool, device=DEV)
    assert ops.lpips_sums(gt, image, weights.packed, none).cpu().tolist() == [0.0] * 5
    assert ops.lpips_sums(gt, gt.clone(), weights.packed).cpu().tolist() == [0.0] * 5
    first = qa.lpips_metrics(image, gt, weights, dev(c['mask']))
    assert first == qa.lpips_metrics(image, gt, weights, dev(c['mask']))
    assert qa.lpips_metrics(image, gt, weights, none) == {'LPIPS': first['LPIPS'], 'MaskedLPIPS': 0.0}
    assert qa.lpips_metrics(gt, gt, weights) == {'LPIPS': 0.0}
    assert qa.lpips_metrics(gt, image, weights)['LPIPS'] == first['LPIPS']


def test_scaling_buffers_are_used():
    """scaling_layer.* of the checkpoint replaces the constants: another shift / scale gives the restatement's other score."""
    from simplenerf_amd import qa
    shape = SHAPES[1]
    c = case(shape)
    other = dict(host_weights(), shift=torch.tensor([0.1, -0.2, 0.05]), scale=torch.tensor([0.5, 0.3, 0.4]))
    want = lpips_reference.lpips(c['gt'], c['image'], other)['score']
    got = qa.lpips_metrics(dev(c['image']), dev(c['gt']), qa.LpipsWeights(other, DEV))['LPIPS']
    print('scaling', got, want, 'default', c['plain']['score'])
    assert abs(want - c['plain']['score']) > 1e-4
    assert abs(got - want) <= min(SUM_TOLERANCE * want, SCORE_CAP)


def test_a_30_pixel_side_raises_before_any_launch():
    from simplenerf_amd import _lib, ops, qa
    weights = device_weights()
    for shape in ((30, 64), (64, 30)):
        image = torch.zeros(shape + (3,), dtype=torch.uint8, device=DEV)
        with pytest.raises(RuntimeError, match=f'AlexNet needs 31 pixels on every side, the image extent is {shape[0]} x {shape[1]}'):
            qa.lpips_metrics(image, image, weights)
        with pytest.raises(RuntimeError, match=f'the image extent is {shape[0]} x {shape[1]}'):
            ops.lpips_sums(image, image, weights.packed)
        # the entry point itself refuses, before enqueuing anything
        lib = _lib.load()
        sums = torch.full((5,), 7.0, dtype=torch.float64, device=DEV)
        scratch = torch.empty((1 << 20,), dtype=torch.uint8, device=DEV)
        status = lib.snerf_lpips_sums(image.data_ptr(), image.data_ptr(), None, shape[0], shape[1], weights.packed.data_ptr(),
                                      sums.data_ptr(), None, scratch.data_ptr(), None)
        assert status != 0 and b'smaller than the network' in lib.snerf_last_error()
        torch.cuda.synchronize()
        assert sums.cpu().tolist() == [7.0] * 5
        assert lib.snerf_lpips_workspace_bytes(shape[0], shape[1]) == 0


def test_evaluate_frames_carries_lpips():
    """With lpips_weights every row carries LPIPS (MaskedLPIPS where the frame has a mask) equal to a direct qa.lpips_metrics call on
    the frame predict_frame renders; without them the table has exactly the keys it had."""
    from simplenerf_amd import harness, qa, synth
    from simplenerf_amd.models.ModelFactory import get_model
    cfg = synth.make_configs('config1')
    model = get_model(cfg, None)
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    model.load_state_dict({k: torch.from_numpy(v) for k, v in synth.synth_state_dict(shapes, 11, 150.0, 4.0).items()})
    model = model.to(DEV).eval()
    h, w = 32, 40
    rng = numpy.random.default_rng(43)
    frames = []
    for i, pose in enumerate((0, 1)):
        frame = {'frame_num': 10 + i, 'camera': synth.camera('fern', pose, resolution=(h, w)),
                 'image': rng.integers(0, 256, (h, w, 3), dtype=numpy.uint8), 'depth': rng.uniform(1.0, 8.0, (h, w)).astype(numpy.float32)}
        if i == 1:
            frame['mask'] = rng.random((h, w)) < 0.6
        frames.append(frame)
    weights = device_weights()
    without = harness.evaluate_frames(model, cfg, frames, torch.device(DEV))
    table = harness.evaluate_frames(model, cfg, frames, torch.device(DEV), lpips_weights=weights)
    image_keys = ['PSNR', 'RMSE', 'SSIM']
    depth_keys = ['DepthMAE', 'DepthRMSE', 'DepthSROCC']
    assert sorted(without['unrounded'][0]) == sorted(image_keys + depth_keys + ['frame_num'])
    assert sorted(without['unrounded'][1]) == sorted(image_keys + depth_keys + ['Masked' + k for k in image_keys + depth_keys] + ['frame_num'])
    assert sorted(without['average']) == sorted(without['unrounded'][1].keys() - {'frame_num'})
    for row, plain, rounded, frame in zip(table['unrounded'], without['unrounded'], table['frames'], frames):
        assert all(row[k] == v or (v != v and row[k] != row[k]) for k, v in plain.items())      # (nan counts as equal to nan)
        assert sorted(set(row) - set(plain)) == (['LPIPS', 'MaskedLPIPS'] if 'mask' in frame else ['LPIPS'])
        out = harness.predict_frame(model, cfg, frame['camera'], torch.device(DEV))
        assert out['image'].std() > 1
        direct = qa.lpips_metrics(dev(out['image']), dev(frame['image']), weights, dev(frame['mask']) if 'mask' in frame else None)
        print(frame['frame_num'], direct)
        assert {k: row[k] for k in direct} == direct and direct['LPIPS'] > 0
        assert all(rounded[k] == qa.round4(direct[k]) for k in direct)
    assert table['average']['LPIPS'] == qa.round4(numpy.mean([r['LPIPS'] for r in table['frames']]))
    assert table['average']['MaskedLPIPS'] == table['frames'][1]['MaskedLPIPS']
