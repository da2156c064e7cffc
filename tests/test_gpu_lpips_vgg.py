"""LPIPS on the VGG-16 backbone on the device (csrc/lpips.hip -> ops.lpips_sums(net='vgg') -> qa.lpips_metrics ->
harness.evaluate_frames) against the float64 restatement of the package's definition (tests/lpips_vgg_reference.py), and the
AlexNet path's results against what it returned before the VGG-16 backbone shared its kernels (tests/golden/lpips_alex_sums.npz).

Tolerances.  The package computes LPIPS in float32, so its precision class is the distance of the float32 restatement from the
float64 one over the four test shapes with the seeded inputs of lpips_vgg_reference (measured by its precision_class on the CPU;
tests/test_lpips_vgg_host.py measures it again and compares with the figures committed here):
  * FEATURE_MEASURED = 7.51e-7   max over shapes and taps of max|x32 - x64| / max|x64|; the gate is 4 x that: another, equally valid
    order of the k sum on the matrix cores against the CPU's blocked convolution -- it does not admit a 16-bit operand (2^-9);
  * SUM_MEASURED = 8.47e-7       max over shapes and layers of |s32 - s64| / |s64|; the gate is 8 x that: one scalar's deviation is a
    noisier sample than a maximum over thousands of elements;
  * the score is also within 5e-5 absolute, half a unit of the 4th decimal the reference's scripts round to.
These are the margins of tests/test_gpu_lpips.py.  Reached on an MI355X: DESIGN.md, "LPIPS"."""
import functools
import os

import numpy
import pytest
import torch

from tests import lpips_reference
from tests import lpips_vgg_reference as reference

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
FEATURE_MEASURED = 7.505499279840569e-07
SUM_MEASURED = 8.46701783300457e-07
FEATURE_TOLERANCE = 4 * FEATURE_MEASURED
SUM_TOLERANCE = 8 * SUM_MEASURED
SCORE_CAP = 5e-5
SHAPES = reference.SHAPES
GOLDEN_ALEX = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'lpips_alex_sums.npz')


def dev(array):
    return torch.as_tensor(array).to(DEV)


@functools.lru_cache(maxsize=None)
def device_weights():
    from simplenerf_amd import qa
    return qa.LpipsWeights(reference.host_weights(), DEV, net='vgg')


@functools.lru_cache(maxsize=None)
def alex_weights():
    from simplenerf_amd import qa
    return qa.LpipsWeights(lpips_reference.random_weights(), DEV)


def sums_of(gt, image, mask=None, **more):
    from simplenerf_amd import ops
    return ops.lpips_sums(gt, image, device_weights().packed, mask, net='vgg', **more)


def score_of(sums, shape):
    from simplenerf_amd import ops
    return float(sum(numpy.float64(s) / (th * tw) for s, (th, tw, _) in zip(sums, ops.lpips_tap_shapes(*shape, net='vgg'))))


@pytest.mark.parametrize('shape', SHAPES)
def test_taps_equal_the_restatement(shape):
    """Every one of the five taps of both images: a wrong pad, pool window, tail, tap order or ping-pong region shows here."""
    from simplenerf_amd import ops
    c = reference.case(shape)
    _, taps = sums_of(dev(c['gt']), dev(c['image']), return_taps=True)
    assert ops.lpips_tap_shapes(*shape, net='vgg') == [(shape[0] >> t, shape[1] >> t, ch) for t, ch in enumerate(reference.TAP_CHANNELS)]
    assert [tuple(t.shape) for t in taps] == [(2, th, tw, ch) for th, tw, ch in ops.lpips_tap_shapes(*shape, net='vgg')]
    for layer, (got, want) in enumerate(zip(taps, c['plain']['taps'])):
        got = got.permute(0, 3, 1, 2).double().cpu()
        assert got.shape == want.shape
        worst = float((got - want).abs().max() / want.abs().max())
        print(shape, 'tap', layer, tuple(want.shape), 'max|x - x64| / max|x64| =', worst, 'active', float((want > 0).double().mean()))
        assert worst <= FEATURE_TOLERANCE


@pytest.mark.parametrize('shape', SHAPES)
def test_sums_and_score_equal_the_restatement(shape):
    from simplenerf_amd import qa
    c = reference.case(shape)
    for name, mask in (('plain', None), ('masked', c['mask'])):
        want = c[name]
        sums = sums_of(dev(c['gt']), dev(c['image']), None if mask is None else dev(mask)).cpu().numpy()
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
    """Two calls and the two argument orders return the same bits; an all-true mask = the plain sums bit for bit; an all-false mask
    and identical images = 0.0 exactly.  (No atomics and no split of K: nothing in the sums depends on the grid or on timing.)"""
    from simplenerf_amd import qa
    c = reference.case(shape)
    gt, image, weights = dev(c['gt']), dev(c['image']), device_weights()
    plain = sums_of(gt, image).cpu().numpy()
    assert numpy.all(plain > 0)
    assert numpy.array_equal(plain, sums_of(gt, image).cpu().numpy())
    assert numpy.array_equal(plain, sums_of(image, gt).cpu().numpy())
    assert numpy.array_equal(plain, sums_of(gt, image, torch.ones(shape, dtype=torch.bool, device=DEV)).cpu().numpy())
    assert numpy.array_equal(plain, sums_of(gt, image, torch.ones(shape, dtype=torch.uint8, device=DEV)).cpu().numpy())
    none = torch.zeros(shape, dtype=torch.bool, device=DEV)
    assert sums_of(gt, image, none).cpu().tolist() == [0.0] * 5
    assert sums_of(gt, gt.clone()).cpu().tolist() == [0.0] * 5
    first = qa.lpips_metrics(image, gt, weights, dev(c['mask']))
    assert first == qa.lpips_metrics(image, gt, weights, dev(c['mask']))
    assert qa.lpips_metrics(image, gt, weights, none) == {'LPIPS': first['LPIPS'], 'MaskedLPIPS': 0.0}
    assert qa.lpips_metrics(gt, gt, weights) == {'LPIPS': 0.0}
    assert qa.lpips_metrics(gt, image, weights)['LPIPS'] == first['LPIPS']


def test_scaling_buffers_are_used():
    """scaling_layer.* of the checkpoint replaces the constants: another shift / scale gives the restatement's other score."""
    from simplenerf_amd import qa
    shape = SHAPES[1]
    c = reference.case(shape)
    other = dict(reference.host_weights(), shift=torch.tensor([0.1, -0.2, 0.05]), scale=torch.tensor([0.5, 0.3, 0.4]))
    want = reference.lpips(c['gt'], c['image'], other)['score']
    got = qa.lpips_metrics(dev(c['image']), dev(c['gt']), qa.LpipsWeights(other, DEV, net='vgg'))['LPIPS']
    print('scaling', got, want, 'default', c['plain']['score'])
    assert abs(want - c['plain']['score']) > 1e-4
    assert abs(got - want) <= min(SUM_TOLERANCE * want, SCORE_CAP)


def test_a_15_pixel_side_raises_before_any_launch():
    from simplenerf_amd import _lib, ops, qa
    weights = device_weights()
    for shape in ((15, 64), (64, 15)):
        image = torch.zeros(shape + (3,), dtype=torch.uint8, device=DEV)
        with pytest.raises(RuntimeError, match=f'gt_image: VGG-16 needs 16 pixels on every side, the image extent is {shape[0]} x {shape[1]}'):
            qa.lpips_metrics(image, image, weights)
        with pytest.raises(RuntimeError, match=f'VGG-16 needs 16 pixels on every side, the image extent is {shape[0]} x {shape[1]}'):
            ops.lpips_sums(image, image, weights.packed, net='vgg')
        # the entry point itself refuses, before enqueuing anything
        lib = _lib.load()
        sums = torch.full((5,), 7.0, dtype=torch.float64, device=DEV)
        scratch = torch.empty((1 << 20,), dtype=torch.uint8, device=DEV)
        status = lib.snerf_lpips_net_sums(1, image.data_ptr(), image.data_ptr(), None, shape[0], shape[1], weights.packed.data_ptr(),
                                          sums.data_ptr(), None, scratch.data_ptr(), None)
        error = lib.snerf_last_error()
        assert status != 0 and b'smaller than the network' in error and f'{shape[0]} x {shape[1]}'.encode() in error
        torch.cuda.synchronize()
        assert sums.cpu().tolist() == [7.0] * 5
        assert lib.snerf_lpips_net_workspace_bytes(1, shape[0], shape[1]) == 0
    # an unknown selector is refused in the same way
    image = torch.zeros((64, 64, 3), dtype=torch.uint8, device=DEV)
    sums = torch.full((5,), 7.0, dtype=torch.float64, device=DEV)
    scratch = torch.empty((1 << 20,), dtype=torch.uint8, device=DEV)
    assert _lib.load().snerf_lpips_net_sums(2, image.data_ptr(), image.data_ptr(), None, 64, 64, weights.packed.data_ptr(), sums.data_ptr(), None,
                                            scratch.data_ptr(), None) != 0
    assert b'network 2' in _lib.load().snerf_last_error()
    torch.cuda.synchronize()
    assert sums.cpu().tolist() == [7.0] * 5


def test_both_backbones_in_one_process():
    """An AlexNet and a VGG-16 LpipsWeights used alternately each keep their own results: a workspace shared between the networks or
    a mix-up of the packed layouts would show."""
    from simplenerf_amd import ops, qa
    shape = (64, 80)
    c = reference.case(shape)
    gt, image, mask = dev(c['gt']), dev(c['image']), dev(c['mask'])
    alex, vgg = alex_weights(), device_weights()
    assert (alex.net, vgg.net) == ('alex', 'vgg') and alex.packed.numel() != vgg.packed.numel()
    want_alex = lpips_reference.lpips(c['gt'], c['image'], lpips_reference.random_weights())['score']
    first = [qa.lpips_metrics(image, gt, weights, mask) for weights in (alex, vgg, alex, vgg)]
    assert first[0] == first[2] and first[1] == first[3] and first[0] != first[1]
    assert abs(first[0]['LPIPS'] - want_alex) <= 5e-5 and abs(first[1]['LPIPS'] - c['plain']['score']) <= 5e-5
    assert abs(want_alex - c['plain']['score']) > 1e-3
    # interleaved on the stream without a synchronisation in between
    sums = [ops.lpips_sums(gt, image, w.packed, net=w.net) for w in (vgg, alex, vgg, alex)]
    assert torch.equal(sums[0], sums[2]) and torch.equal(sums[1], sums[3])
    # a buffer packed for the other network is refused by its size
    with pytest.raises(RuntimeError, match='packed: expected shape'):
        ops.lpips_sums(gt, image, alex.packed, net='vgg')
    with pytest.raises(RuntimeError, match='packed: expected shape'):
        ops.lpips_sums(gt, image, vgg.packed)


def test_evaluate_frames_carries_vgg_lpips():
    """With VGG-16 weights every row carries LPIPS (MaskedLPIPS where the frame has a mask) equal to a direct qa.lpips_metrics call
    on the frame predict_frame renders; without weights the table has exactly the keys it had."""
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
    for row, plain, rounded, frame in zip(table['unrounded'], without['unrounded'], table['frames'], frames):
        assert all(row[k] == v or (v != v and row[k] != row[k]) for k, v in plain.items())      # (nan counts as equal to nan)
        assert sorted(set(row) - set(plain)) == (['LPIPS', 'MaskedLPIPS'] if 'mask' in frame else ['LPIPS'])
        out = harness.predict_frame(model, cfg, frame['camera'], torch.device(DEV))
        direct = qa.lpips_metrics(dev(out['image']), dev(frame['image']), weights, dev(frame['mask']) if 'mask' in frame else None)
        print(frame['frame_num'], direct)
        assert {k: row[k] for k in direct} == direct and direct['LPIPS'] > 0
        assert all(rounded[k] == qa.round4(direct[k]) for k in direct)
        # it is the VGG-16 score, not the AlexNet one under the same key
        assert direct['LPIPS'] != qa.lpips_metrics(dev(out['image']), dev(frame['image']), alex_weights())['LPIPS']
    assert table['average']['LPIPS'] == qa.round4(numpy.mean([r['LPIPS'] for r in table['frames']]))
    assert table['average']['MaskedLPIPS'] == table['frames'][1]['MaskedLPIPS']


def test_alexnet_sums_equal_the_recorded_ones():
    """The five layer sums, plain and masked, of the four AlexNet cases are bit for bit what the AlexNet-only kernels returned on an
    MI355X (tools/make_golden_lpips_alex.py): sharing the convolution, the pool and the entry points with VGG-16 moved nothing."""
    from simplenerf_amd import ops
    golden = numpy.load(GOLDEN_ALEX)
    assert sorted(golden.files) == sorted(f'{kind}_{h}x{w}' for kind in ('plain', 'masked') for h, w in lpips_reference.SHAPES)
    weights = alex_weights()
    for h, w in lpips_reference.SHAPES:
        gt, image, mask = (dev(a) for a in lpips_reference.random_images(h, w))
        plain = ops.lpips_sums(gt, image, weights.packed).cpu().numpy()
        masked = ops.lpips_sums(gt, image, weights.packed, mask).cpu().numpy()
        print(h, w, plain.tolist(), masked.tolist())
        assert golden[f'plain_{h}x{w}'].dtype == numpy.float64 and golden[f'plain_{h}x{w}'].shape == (5,)
        assert numpy.array_equal(plain, golden[f'plain_{h}x{w}'])
        assert numpy.array_equal(masked, golden[f'masked_{h}x{w}'])
        assert numpy.array_equal(ops.lpips_sums(gt, image, weights.packed, net='alex').cpu().numpy(), golden[f'plain_{h}x{w}'])
