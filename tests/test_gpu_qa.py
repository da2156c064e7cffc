"""Frame metrics on the device (csrc/metrics.hip -> ops -> qa -> harness.evaluate_frames) against the host restatement of the
reference's QA scripts (tests/qa_reference.py).  Both sides compute in fp64, so the tolerances follow from the arithmetic:
image error sums are exact integers (RMSE / PSNR compare with ==), SSIM and the S map 1e-9 absolute, depth sums 1e-12
relative, SROCC 1e-10 absolute."""
import math
import os
import socket
import subprocess
import sys

import numpy
import pytest
import torch

from tests import qa_reference

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def dev(array):
    return torch.as_tensor(array).to(DEV)


def random_pair(h, w, seed):
    rng = numpy.random.default_rng(seed)
    return rng.integers(0, 256, (h, w, 3), dtype=numpy.uint8), rng.integers(0, 256, (h, w, 3), dtype=numpy.uint8)


def smooth_pair(h=64, w=80):
    """Bright and smooth: E[x^2] ~ 53 000 against C2 = 58.5 -- an fp32 evaluation of the variance is ~3e-6 off here."""
    y, x = numpy.mgrid[0:h, 0:w]
    base = 230 + 10 * numpy.sin(x / 9) + 5 * numpy.cos(y / 7)
    noise = numpy.random.default_rng(5).integers(-2, 3, (h, w, 3))
    gt = numpy.round(numpy.stack([base] * 3, 2)).astype(numpy.uint8)
    image = numpy.clip(numpy.round(numpy.stack([base] * 3, 2)) + noise, 0, 255).astype(numpy.uint8)
    return gt, image


def check_image(gt, image, mask=None):
    """Device metrics, exact sums and the S map of one pair against the restatement; returns the device metrics."""
    from simplenerf_amd import ops, qa
    got = qa.image_metrics(dev(image), dev(gt), None if mask is None else dev(mask))
    want = qa_reference.image_metrics(image, gt, mask)
    print({k: (got[k], want[k]) for k in want})
    sums = ops.image_error_sums(dev(gt), dev(image), None if mask is None else dev(mask)).cpu().tolist()
    assert tuple(sums) == qa_reference.error_sums(image, gt, mask)
    qa_reference.assert_close(got, want)
    s_map = qa.ssim_map(dev(image), dev(gt)).cpu().numpy()
    worst = numpy.abs(s_map - qa_reference.ssim_map(gt, image)).max()
    print('S map', worst)
    assert worst <= 1e-9
    return got


@pytest.mark.parametrize('shape', [(11, 11), (37, 53), (64, 64), (75, 139)])
def test_image_metrics_random_content(shape):
    """11x11: the crop leaves one pixel and every tap of the corner pixels is reflected; 37x53: ragged both ways; 64x64: whole
    tiles; 75x139: several tiles each way with ragged edges.  With a random mask."""
    gt, image = random_pair(*shape, seed=shape[0])
    mask = numpy.random.default_rng(shape[1]).random(shape) < 0.4
    check_image(gt, image, mask)


def test_image_metrics_bright_smooth_image_needs_fp64():
    gt, image = smooth_pair()
    check_image(gt, image)


def test_constant_images_equal_the_closed_form():
    from simplenerf_amd import qa
    a, b, c1 = 100.0, 110.0, 6.5025
    want = (2 * a * b + c1) / (a * a + b * b + c1)
    gt = torch.full((23, 31, 3), 100, dtype=torch.uint8, device=DEV)
    image = torch.full((23, 31, 3), 110, dtype=torch.uint8, device=DEV)
    assert abs(qa.image_metrics(image, gt)['SSIM'] - want) <= 1e-12
    assert float((qa.ssim_map(image, gt) - want).abs().max()) <= 1e-12


def test_masks():
    from simplenerf_amd import qa
    gt, image = random_pair(37, 53, seed=11)
    full = numpy.ones((37, 53), dtype=bool)
    got = check_image(gt, image, full)
    assert got['MaskedRMSE'] == got['RMSE'] and got['MaskedPSNR'] == got['PSNR']
    border = numpy.zeros((37, 53), dtype=bool)
    border[36, 0] = True                                       # a single border pixel: every vertical tap below it is reflected
    check_image(gt, image, border)
    empty = numpy.zeros((37, 53), dtype=bool)
    got = qa.image_metrics(dev(image), dev(gt), dev(empty))
    assert all(math.isnan(got[k]) for k in ('MaskedRMSE', 'MaskedPSNR', 'MaskedSSIM')) and not math.isnan(got['SSIM'])
    # a uint8 0/1 mask is the same mask
    random_mask = numpy.random.default_rng(2).random((37, 53)) < 0.5
    assert qa.image_metrics(dev(image), dev(gt), dev(random_mask)) == qa.image_metrics(dev(image), dev(gt), dev(random_mask.astype(numpy.uint8)))


def test_identical_images():
    from simplenerf_amd import qa
    gt, _ = random_pair(37, 53, seed=3)
    got = qa.image_metrics(dev(gt), dev(gt), dev(numpy.ones((37, 53), dtype=bool)))
    assert got['PSNR'] == math.inf and got['MaskedPSNR'] == math.inf and got['RMSE'] == 0.0
    assert abs(got['SSIM'] - 1) <= 1e-12 and abs(got['MaskedSSIM'] - 1) <= 1e-12


def depth_cases():
    rng = numpy.random.default_rng(17)
    h, w = 37, 53                                              # 1961 pixels: odd
    gt = rng.uniform(0.5, 9.0, (h, w)).astype(numpy.float32)
    noisy = (gt * rng.uniform(0.8, 1.25, (h, w)) + rng.normal(0, 0.3, (h, w))).astype(numpy.float32)
    quantised = (numpy.round(noisy * 4) / 4).astype(numpy.float32)            # ~40 distinct values: long tie runs
    zeros = numpy.maximum(noisy, 0)
    zeros.reshape(-1)[:(h * w) // 3] = 0.0                                     # a block of exact zeros (a depth clipped at 0)
    mask = rng.random((h, w)) < 0.45
    return {'plain': (gt, noisy, mask), 'ties': (numpy.round(gt * 2).astype(numpy.float32) / 2, quantised, mask),
            'zeros': (gt, zeros.astype(numpy.float32), mask),
            'even': (gt[:, :52].copy(), noisy[:, :52].copy(), mask[:, :52].copy())}      # 1924 pixels: even (median of two)


@pytest.mark.parametrize('case', ['plain', 'ties', 'zeros', 'even'])
def test_depth_metrics(case):
    from simplenerf_amd import qa
    gt, depth, mask = depth_cases()[case]
    for m in (None, mask):
        got = qa.depth_metrics(dev(depth), dev(gt), eval_scale=1.0 / 1.7, gt_scale=1.0 / 2.3, mask=None if m is None else dev(m))
        want = qa_reference.depth_metrics(depth, gt, 1.0 / 1.7, 1.0 / 2.3, m)
        print(case, {k: (got[k], want[k]) for k in want})
        qa_reference.assert_close(got, want)


def test_depth_metrics_empty_mask_and_constant_side():
    from simplenerf_amd import qa
    gt, depth, mask = depth_cases()['plain']
    got = qa.depth_metrics(dev(depth), dev(gt), mask=dev(numpy.zeros_like(mask)))
    assert all(math.isnan(got[k]) for k in ('MaskedDepthRMSE', 'MaskedDepthMAE', 'MaskedDepthSROCC'))
    assert not any(math.isnan(got[k]) for k in ('DepthRMSE', 'DepthMAE', 'DepthSROCC'))
    assert math.isnan(qa.depth_metrics(dev(numpy.full_like(depth, 2.0)), dev(gt))['DepthSROCC'])     # scipy: nan for a constant input


@pytest.fixture(scope='module')
def large_pair():
    """378 x 504: 12 x 24 SSIM tiles (a two-dimensional grid), 745 workgroups in the flat reductions."""
    h, w = 378, 504
    rng = numpy.random.default_rng(23)
    y, x = numpy.mgrid[0:h, 0:w]
    gt = numpy.clip(128 + 90 * numpy.sin(x / 23)[..., None] * numpy.cos(y / 31)[..., None] + rng.normal(0, 12, (h, w, 3)), 0, 255).astype(numpy.uint8)
    image = numpy.clip(gt.astype(numpy.float64) + rng.normal(0, 6, (h, w, 3)), 0, 255).astype(numpy.uint8)
    gt_depth = (3 + numpy.sin(x / 40) + 0.5 * numpy.cos(y / 17) + rng.normal(0, 0.05, (h, w))).astype(numpy.float32)
    depth = numpy.maximum(gt_depth * 1.1 + rng.normal(0, 0.2, (h, w)) - 2.2, 0).astype(numpy.float32)      # part of it clipped at 0
    mask = rng.random((h, w)) < 0.7
    return gt, image, gt_depth, depth, mask


def test_half_size_frame_all_metrics(large_pair):
    from simplenerf_amd import qa
    gt, image, gt_depth, depth, mask = large_pair
    check_image(gt, image, mask)
    got = qa.depth_metrics(dev(depth), dev(gt_depth), 0.9, 1.1, dev(mask))
    want = qa_reference.depth_metrics(depth, gt_depth, 0.9, 1.1, mask)
    print({k: (got[k], want[k]) for k in want})
    qa_reference.assert_close(got, want)


def test_two_calls_return_identical_bits(large_pair):
    from simplenerf_amd import ops, qa
    gt, image, gt_depth, depth, mask = (dev(a) for a in large_pair)
    first = (qa.image_metrics(image, gt, mask), qa.depth_metrics(depth, gt_depth, 0.9, 1.1, mask))
    sums, s_map = ops.ssim_sums(gt, image, mask, return_map=True)
    second = (qa.image_metrics(image, gt, mask), qa.depth_metrics(depth, gt_depth, 0.9, 1.1, mask))
    sums2, s_map2 = ops.ssim_sums(gt, image, mask, return_map=True)
    assert first == second                                     # dicts of Python floats: == is bit equality (no nan in here)
    assert torch.equal(sums, sums2) and torch.equal(s_map, s_map2)


# ------------------------------------------------------------------------------------------------ evaluate_frames
def tiny_model_and_frames(kind='config1'):
    """Two 24 x 32 frames with synthetic targets, depths and (on the second) a mask.  'config1': BASELINE config 1's shapes (4x128
    coarse MLP, 64 samples, world-space rays) with a random field that is neither empty nor dead.  'config2': the 8x256 coarse + fine NDC renderer with the opaque random field of the
    driver's smoke run (fine MLP = coarse MLP), whose frames are known not to be empty."""
    from simplenerf_amd import synth
    from simplenerf_amd.models.ModelFactory import get_model
    cfg = synth.make_configs(kind)
    model = get_model(cfg, None)
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    seed, gain, shift = (11, 150.0, 4.0) if kind == 'config1' else (7, 200.0, 8.0)
    sd = {k: torch.from_numpy(v) for k, v in synth.synth_state_dict(shapes, seed, gain, shift).items()}
    for k in list(sd):
        if k.startswith('coarse_model.') and 'fine_mlp' in cfg['model']:
            sd['fine_model.' + k[len('coarse_model.'):]] = sd[k].clone()
    model.load_state_dict(sd)
    model = model.to(DEV).eval()
    rng = numpy.random.default_rng(41)
    frames = []
    for i, pose in enumerate((0, 1)):
        cam = synth.camera('fern', pose, resolution=(24, 32))
        frame = {'frame_num': 10 + i, 'camera': cam, 'image': rng.integers(0, 256, (24, 32, 3), dtype=numpy.uint8),
                 'depth': rng.uniform(1.0, 8.0, (24, 32)).astype(numpy.float32), 'depth_scale': 0.5, 'gt_depth_scale': 0.25}
        if i == 1:
            frame['mask'] = rng.random((24, 32)) < 0.6
        frames.append(frame)
    return cfg, model, frames


def same(a, b):
    """Equal, nan counting as equal to nan."""
    return a == b or (isinstance(a, float) and isinstance(b, float) and math.isnan(a) and math.isnan(b))


def check_table(table, cfg, model, frames):
    from simplenerf_amd import harness
    assert sorted(table) == ['average', 'frames', 'unrounded']
    assert [r['frame_num'] for r in table['frames']] == [10, 11]
    for row, rounded, frame in zip(table['unrounded'], table['frames'], frames):
        out = harness.predict_frame(model, cfg, frame['camera'], torch.device(DEV))
        mask = frame.get('mask')
        print(frame['frame_num'], 'distinct depths', numpy.unique(out['depth']).size, 'image std', float(out['image'].std()))
        # the frames must exercise the metrics: a constant render has no rank correlation and no structure to compare
        assert numpy.unique(out['depth']).size > 100 and out['image'].std() > 1
        want = qa_reference.image_metrics(out['image'], frame['image'], mask)
        want.update(qa_reference.depth_metrics(out['depth'], frame['depth'], frame['depth_scale'], frame['gt_depth_scale'], mask))
        got = {k: v for k, v in row.items() if k != 'frame_num'}
        print(frame['frame_num'], {k: (got[k], want[k]) for k in want})
        qa_reference.assert_close(got, want)
        assert sorted(rounded) == sorted(row)
        assert all(same(rounded[k], v if k == 'frame_num' else float(numpy.round(v, 4))) for k, v in row.items())
    assert 'MaskedSSIM' not in table['frames'][0] and 'MaskedSSIM' in table['frames'][1]
    for name, value in table['average'].items():
        values = [r[name] for r in table['frames'] if name in r]
        assert same(value, float(numpy.round(numpy.mean(values), 4))), name
    assert sorted(table['average']) == sorted(table['frames'][1].keys() - {'frame_num'})


@pytest.mark.parametrize('kind', ['config1', 'config2'])
def test_evaluate_frames_scores_what_predict_frame_renders(kind):
    from simplenerf_amd import harness
    cfg, model, frames = tiny_model_and_frames(kind)
    check_table(harness.evaluate_frames(model, cfg, frames, torch.device(DEV)), cfg, model, frames)


_COLLECTIVE_WORKER = r'''
import sys
sys.path.insert(0, sys.argv[1])
import torch
import torch.distributed as dist
from simplenerf_amd import harness
from tests import test_gpu_qa
dev = torch.device('cuda', 0)
torch.cuda.set_device(dev)
dist.init_process_group('nccl', rank=0, world_size=1, device_id=dev)
for kind in ('config1', 'config2'):
    cfg, model, frames = test_gpu_qa.tiny_model_and_frames(kind)
    table = harness.evaluate_frames(model, cfg, frames, dev, rank=0, world_size=1, collective=True)
    test_gpu_qa.check_table(table, cfg, model, frames)
    plain = harness.evaluate_frames(model, cfg, frames, dev)
    assert repr(plain) == repr(table)
torch.cuda.synchronize()
dist.barrier()
dist.destroy_process_group()
print('evaluate_frames collective: OK')
'''


def test_evaluate_frames_through_a_one_rank_gather():
    """``collective=True`` on a one-rank RCCL group (a fresh process, as tests/test_gpu_dist.py does): every frame reaches rank 0
    through harness.gather_rays, rank 0 returns the table, and it is the table of the plain call."""
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        port = s.getsockname()[1]
    env = {k: v for k, v in os.environ.items() if k not in ('RANK', 'LOCAL_RANK', 'WORLD_SIZE', 'MASTER_ADDR', 'MASTER_PORT')}
    env.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')
    env.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    r = subprocess.run([sys.executable, '-c', _COLLECTIVE_WORKER, repo], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and 'evaluate_frames collective: OK' in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
