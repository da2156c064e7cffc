"""Host side of LPIPS on the VGG-16 backbone (qa.lpips_metrics with net='vgg', csrc/lpips.hip): the checkpoint loader, the
restatement the metric is pinned to (tests/lpips_vgg_reference.py) and the conditions its seeded inputs must meet, the VGG-16 index
arithmetic and workspace plan of csrc/conv_index.h walked on the host under sanitizers, the exported symbols, the refusals and the
measured tolerance constants of tests/test_gpu_lpips_vgg.py -- none of it needs a GPU."""
import ctypes
import os
import subprocess

import numpy
import pytest
import torch

from simplenerf_amd import _lib, ops, qa
from tests import lpips_reference, test_gpu_lpips_vgg
from tests import lpips_vgg_reference as reference

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('snerf_lpips_net_packed_floats', 'snerf_lpips_net_pack', 'snerf_lpips_net_workspace_bytes', 'snerf_lpips_net_tap_shape',
         'snerf_lpips_net_sums')
FEATURES = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)
SLICES = (1, 1, 2, 2, 3, 3, 3, 4, 4, 4, 5, 5, 5)
CHANNELS = ((3, 64), (64, 64), (64, 128), (128, 128), (128, 256), (256, 256), (256, 256), (256, 512), (512, 512), (512, 512), (512, 512),
            (512, 512), (512, 512))


def checkpoints():
    """The same 13 + 13 + 5 tensors in both layouts, built here: (a saved lpips.LPIPS(net='vgg') state dict, torchvision's vgg16,
    vgg.pth, tensors)."""
    tensors = reference.random_weights(5)
    package, torchvision, lin = {}, {}, {}
    for l, (s, i) in enumerate(zip(SLICES, FEATURES)):
        for part, group in (('weight', 'conv_weights'), ('bias', 'conv_biases')):
            package[f'net.slice{s}.{i}.{part}'] = tensors[group][l].clone()
            torchvision[f'features.{i}.{part}'] = tensors[group][l].clone()
    for t in range(5):
        lin[f'lin{t}.model.1.weight'] = tensors['lin_weights'][t].reshape(1, -1, 1, 1).clone()
        package[f'lin{t}.model.1.weight'] = lin[f'lin{t}.model.1.weight'].clone()
        package[f'lins.{t}.model.1.weight'] = lin[f'lin{t}.model.1.weight'].clone()
    package['scaling_layer.shift'] = torch.tensor(reference.SHIFT).reshape(1, 3, 1, 1)
    package['scaling_layer.scale'] = torch.tensor(reference.SCALE).reshape(1, 3, 1, 1)
    torchvision['classifier.0.weight'] = torch.zeros(8, 8)          # ignored
    torchvision['classifier.0.bias'] = torch.zeros(8)
    return package, torchvision, lin, tensors


def same_tensors(got, want):
    return all(len(got[g]) == n and all(torch.equal(a, b) and a.dtype == torch.float32 for a, b in zip(got[g], want[g]))
               for g, n in (('conv_weights', 13), ('conv_biases', 13), ('lin_weights', 5))) and all(torch.equal(got[k], want[k]) for k in ('shift', 'scale'))


def test_the_network_is_the_stated_one():
    assert reference.FEATURE_INDICES == FEATURES and ops.LPIPS_VGG_TAP_CONVS == (1, 3, 6, 9, 12) and ops.LPIPS_VGG_MIN_EXTENT == 16
    assert tuple((c_in, c_out) for c_out, c_in, _, _ in reference.CONVS) == CHANNELS
    assert tuple((c_in, c_out) for c_out, c_in, k in ops.LPIPS_VGG_CONVS) == CHANNELS and all(k == 3 for _, _, k in ops.LPIPS_VGG_CONVS)
    assert [l for l, conv in enumerate(reference.CONVS) if conv[2]] == [2, 4, 7, 10]              # the pools at features 4, 9, 16, 23
    assert [FEATURES[l] for l, conv in enumerate(reference.CONVS) if conv[3] is not None] == [2, 7, 14, 21, 28]
    assert [reference.CONVS[l][0] for l in ops.LPIPS_VGG_TAP_CONVS] == list(reference.TAP_CHANNELS) == [64, 128, 256, 512, 512]
    # the AlexNet names keep their meaning
    assert ops.LPIPS_MIN_EXTENT == 31 and ops.LPIPS_CONVS == ((64, 3, 11), (192, 64, 5), (384, 192, 3), (256, 384, 3), (256, 256, 3))
    # 305 856 multiply-accumulates per image pixel: every pool divides the pixels by four
    pools, macs = 0, 0.0
    for (c_in, c_out), conv in zip(CHANNELS, reference.CONVS):
        pools += conv[2]
        macs += 9 * c_in * c_out / 4 ** pools
    assert macs == 305856


def test_both_checkpoint_layouts_give_the_same_tensors(tmp_path):
    package, torchvision, lin, tensors = checkpoints()
    assert same_tensors(qa.lpips_tensors(package, net='vgg'), tensors)
    assert same_tensors(qa.lpips_tensors(torchvision, lin, net='vgg'), tensors)
    assert [tuple(t.shape) for t in qa.lpips_tensors(package, net='vgg')['lin_weights']] == [(64,), (128,), (256,), (512,), (512,)]
    # only the `lins.{k}` duplicates present; float64 tensors are converted
    renamed = {k: v.double() for k, v in package.items() if not k.startswith('lin')}
    renamed.update({k: v for k, v in package.items() if k.startswith('lins.')})
    assert same_tensors(qa.lpips_tensors(renamed, net='vgg'), tensors)
    # the files are plain dictionaries of tensors: torch.load(weights_only=True) reads them back
    torch.save(torchvision, tmp_path / 'vgg16.pth')
    torch.save(lin, tmp_path / 'vgg.pth')
    state = torch.load(tmp_path / 'vgg16.pth', map_location='cpu', weights_only=True)
    assert same_tensors(qa.lpips_tensors(state, torch.load(tmp_path / 'vgg.pth', map_location='cpu', weights_only=True), net='vgg'), tensors)
    # scaling_layer.* overrides the constants
    package['scaling_layer.shift'] = torch.tensor([0.1, -0.2, 0.05]).reshape(1, 3, 1, 1)
    package['scaling_layer.scale'] = torch.tensor([0.5, 0.3, 0.4]).reshape(1, 3, 1, 1)
    got = qa.lpips_tensors(package, net='vgg')
    assert got['shift'].tolist() == torch.tensor([0.1, -0.2, 0.05]).tolist() and got['scale'].tolist() == torch.tensor([0.5, 0.3, 0.4]).tolist()
    assert qa.lpips_tensors(torchvision, lin, net='vgg')['shift'].tolist() == torch.tensor(qa.LPIPS_SHIFT).tolist()


def test_the_loader_names_what_is_wrong():
    package, torchvision, lin, _ = checkpoints()
    with pytest.raises(RuntimeError, match=r'lin0\.model\.1\.weight: missing from the checkpoint'):
        qa.lpips_tensors(torchvision, net='vgg')               # torchvision's file alone has no lin layers
    with pytest.raises(RuntimeError, match=r"neither .*net='vgg'.*net\.slice1\.0\.weight.*vgg16.*features\.0\.weight"):
        qa.lpips_tensors(lin, net='vgg')                       # vgg.pth alone: an unknown layout
    with pytest.raises(RuntimeError, match="net: expected 'alex' or 'vgg', got 'squeeze'"):
        qa.lpips_tensors(package, net='squeeze')
    for key in ('features.2.bias', 'features.28.weight', 'features.17.weight'):
        with pytest.raises(RuntimeError, match=key.replace('.', r'\.') + ': missing from the checkpoint'):
            qa.lpips_tensors({k: v for k, v in torchvision.items() if k != key}, lin, net='vgg')
    with pytest.raises(RuntimeError, match=r'net\.slice4\.19\.weight: missing from the checkpoint'):
        qa.lpips_tensors({k: v for k, v in package.items() if k != 'net.slice4.19.weight'}, net='vgg')
    with pytest.raises(RuntimeError, match=r'lin3\.model\.1\.weight: missing from the checkpoint'):
        qa.lpips_tensors(torchvision, {k: v for k, v in lin.items() if k != 'lin3.model.1.weight'}, net='vgg')
    with pytest.raises(RuntimeError, match=r'features\.5\.weight: expected a tensor of shape \(128, 64, 3, 3\), got \(128, 64, 5, 5\)'):
        qa.lpips_tensors(dict(torchvision, **{'features.5.weight': torch.zeros(128, 64, 5, 5)}), lin, net='vgg')
    with pytest.raises(RuntimeError, match=r'features\.0\.bias: expected a tensor of shape \(64,\), got \(63,\)'):
        qa.lpips_tensors(dict(torchvision, **{'features.0.bias': torch.zeros(63)}), lin, net='vgg')
    with pytest.raises(RuntimeError, match=r'lin2\.model\.1\.weight: expected a tensor of shape \(1, 256, 1, 1\), got \(1, 384, 1, 1\)'):
        qa.lpips_tensors(torchvision, dict(lin, **{'lin2.model.1.weight': torch.zeros(1, 384, 1, 1)}), net='vgg')
    # a file of the other network fails on its first tensor: by shape where the name exists, by name where it does not
    alex = lpips_reference.random_weights(5)
    alex_torchvision = {}
    for l, i in enumerate((0, 3, 6, 8, 10)):
        alex_torchvision[f'features.{i}.weight'] = alex['conv_weights'][l]
        alex_torchvision[f'features.{i}.bias'] = alex['conv_biases'][l]
    alex_lin = {f'lin{l}.model.1.weight': alex['lin_weights'][l].reshape(1, -1, 1, 1) for l in range(5)}
    with pytest.raises(RuntimeError, match=r'features\.0\.weight: expected a tensor of shape \(64, 3, 3, 3\), got \(64, 3, 11, 11\)'):
        qa.lpips_tensors(alex_torchvision, alex_lin, net='vgg')
    with pytest.raises(RuntimeError, match=r'features\.0\.weight: expected a tensor of shape \(64, 3, 11, 11\), got \(64, 3, 3, 3\)'):
        qa.lpips_tensors(torchvision, lin)                     # and VGG-16's file under net='alex'
    with pytest.raises(RuntimeError, match=r'net\.slice1\.0\.weight: expected a tensor of shape \(64, 3, 11, 11\), got \(64, 3, 3, 3\)'):
        qa.lpips_tensors(package)


def test_restatement_identical_images_and_masks():
    weights = reference.host_weights()
    c = reference.case((37, 53))
    gt, image, mask = c['gt'], c['image'], c['mask']
    for dtype in (torch.float64, torch.float32):
        assert reference.lpips(gt, gt, weights, dtype)['score'] == 0.0
        assert reference.lpips(gt, image, weights, dtype, mask=numpy.zeros((37, 53), dtype=bool))['score'] == 0.0
    plain = c['plain']
    assert reference.lpips(gt, image, weights, mask=numpy.ones((37, 53), dtype=bool))['score'] == plain['score']
    assert 0 < c['masked']['score'] < plain['score']
    assert [tuple(t.shape) for t in plain['taps']] == [(2, 64, 37, 53), (2, 128, 18, 26), (2, 256, 9, 13), (2, 512, 4, 6), (2, 512, 2, 3)]
    assert abs(sum(s / (t.shape[2] * t.shape[3]) for s, t in zip(plain['sums'], plain['taps'])) - plain['score']) < 1e-15
    with pytest.raises(ValueError, match='VGG-16 needs 16 pixels on every side, the image extent is 15 x 40'):
        reference.lpips(gt[:15, :40], image[:15, :40], weights)


def test_restatement_on_a_hand_sized_case():
    """The second tap's input chain on a 16 x 16 pair with explicit loops in float64: scaling, conv1_1, conv1_2 (tap 0), the 2 x 2
    floor-mode pool, conv2_1 at a few output pixels, and tap 0's layer sum.  The restatement agrees to 1e-12."""
    weights = reference.random_weights(3)
    gt, image, _ = lpips_reference.random_images(17, 16, seed=9)         # 17 rows: the pool drops the last one
    got = reference.lpips(gt, image, weights)
    shift, scale = weights['shift'].double().numpy(), weights['scale'].double().numpy()

    def conv(x, l):                                                      # x (h, w, c_in) -> (h, w, c_out), 3 x 3, pad 1, bias, ReLU
        w, b = weights['conv_weights'][l].double().numpy(), weights['conv_biases'][l].double().numpy()
        h, wd = x.shape[:2]
        out = numpy.zeros((h, wd, w.shape[0]))
        for oy in range(h):
            for ox in range(wd):
                total = b.copy()
                for ky in range(3):
                    for kx in range(3):
                        iy, ix = oy - 1 + ky, ox - 1 + kx
                        if 0 <= iy < h and 0 <= ix < wd:                 # zero padding otherwise
                            total += w[:, :, ky, kx] @ x[iy, ix]
                out[oy, ox] = numpy.maximum(total, 0.0)
        return out

    features = []
    for frame in (gt, image):
        x = (frame.astype(numpy.float32) * numpy.float32(2) / numpy.float32(255) - numpy.float32(1)).astype(numpy.float64)
        features.append(conv(conv((x - shift) / scale, 0), 1))
    for k in range(2):
        want = features[k].transpose(2, 0, 1)
        assert numpy.abs(got['taps'][0][k].numpy() - want).max() <= 1e-12 * numpy.abs(want).max()
    total = 0.0
    lin = weights['lin_weights'][0].double().numpy()
    for oy in range(17):
        for ox in range(16):
            a, e = features[0][oy, ox], features[1][oy, ox]
            a, e = a / (numpy.sqrt(numpy.sum(a * a)) + 1e-10), e / (numpy.sqrt(numpy.sum(e * e)) + 1e-10)
            total += numpy.sum(lin * (a - e) ** 2)
    assert abs(got['sums'][0] - total) <= 1e-12 * total and abs(got['layers'][0] - total / (17 * 16)) <= 1e-12 * total / (17 * 16)
    pooled = numpy.zeros((8, 8, 64))
    for oy in range(8):
        for ox in range(8):
            pooled[oy, ox] = features[0][2 * oy:2 * oy + 2, 2 * ox:2 * ox + 2].reshape(4, 64).max(axis=0)
    want = conv(conv(pooled, 2), 3).transpose(2, 0, 1)                   # tap 1 of the gt image
    assert got['taps'][1].shape == (2, 128, 8, 8)
    assert numpy.abs(got['taps'][1][0].numpy() - want).max() <= 1e-12 * numpy.abs(want).max()


def test_the_seeded_inputs_meet_their_conditions():
    """Conditions on the inputs, not tolerances: in the float64 restatement every tap of every shape has between 10 % and 90 %
    positive activations, every layer sum is > 0 and every score exceeds 1e-3 (so that relative gates mean something)."""
    assert reference.SHAPES == ((16, 16), (37, 53), (64, 80), (96, 131))
    for shape in reference.SHAPES:
        c = reference.case(shape)
        for name in ('plain', 'masked'):
            active = [float((t > 0).double().mean()) for t in c[name]['taps']]
            print(shape, name, c[name]['score'], c[name]['sums'], active)
            assert all(0.1 <= a <= 0.9 for a in active)
            assert all(s > 0 for s in c[name]['sums'])
            assert c[name]['score'] > 1e-3


def test_conv_index_walk_on_the_host_under_sanitizers(tmp_path):
    """tests/native/conv_index_vgg_test.cpp enumerates every (output pixel, k) of every VGG-16 layer through csrc/conv_index.h for
    the test shapes and a full 756 x 1008 frame, the pool windows and the workspace plan, built with AddressSanitizer + UBSan, as
    its own process."""
    exe = str(tmp_path / 'conv_index_vgg_test')
    r = subprocess.run(['g++', '-O1', '-g', '-std=c++17', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                        os.path.join(REPO, 'tests', 'native', 'conv_index_vgg_test.cpp'), '-o', exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    shapes = reference.SHAPES + ((756, 1008),)
    r = subprocess.run([exe] + [str(v) for shape in shapes for v in shape], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, ASAN_OPTIONS='detect_leaks=0'))
    assert r.returncode == 0 and 'conv_index_vgg_test: OK' in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    assert 'extents 756 x 1008: 756 x 1008 378 x 504 189 x 252 94 x 126 47 x 63\n' in r.stdout
    assert 'extents 16 x 16: 16 x 16 8 x 8 4 x 4 2 x 2 1 x 1\n' in r.stdout
    # the extents the test program derived are those of the restatement's taps
    for h, w in reference.SHAPES:
        want = ' '.join(f'{t.shape[2]} x {t.shape[3]}' for t in reference.case((h, w))['plain']['taps'])
        assert f'extents {h} x {w}: {want}\n' in r.stdout
    # the plan's total is what the library reports, and the figure DESIGN.md states for a full frame
    lib = _lib.load()
    for h, w in shapes:
        assert f'plan {h} x {w}: {lib.snerf_lpips_net_workspace_bytes(1, h, w)} bytes\n' in r.stdout
    assert lib.snerf_lpips_net_workspace_bytes(1, 756, 1008) == 1347019264
    r = subprocess.run([exe, '15', '64'], capture_output=True, text=True, timeout=60, env=dict(os.environ, ASAN_OPTIONS='detect_leaks=0'))
    assert r.returncode == 1 and 'FAILED' in r.stdout


def test_library_exports_the_network_entry_points():
    header = open(os.path.join(REPO, 'include', 'simplenerf_hip.h')).read()
    lib = _lib.load()
    for name in NAMES:
        assert name + '(' in header and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert 'SNERF_LPIPS_ALEX = 0' in header and 'SNERF_LPIPS_VGG16 = 1' in header
    assert lib.snerf_abi_version() == _lib.ABI_VERSION == 10
    # with the selector at ALEX the new entry points answer as the old ones do
    assert lib.snerf_lpips_net_packed_floats(0) == lib.snerf_lpips_packed_floats()
    for h, w in ((31, 31), (30, 64), (756, 1008), (40000, 40000)):
        assert lib.snerf_lpips_net_workspace_bytes(0, h, w) == lib.snerf_lpips_workspace_bytes(h, w)
    assert ops.lpips_tap_shapes(756, 1008, net='alex') == ops.lpips_tap_shapes(756, 1008)
    # shift, scale, padding | W[k_padded][c_out] + bias per convolution | the five lin layers
    k_padded = [-(-(c_in * 9) // 32) * 32 for c_in, _ in CHANNELS]
    assert k_padded[:3] == [32, 576, 576] and k_padded[-1] == 4608
    assert lib.snerf_lpips_net_packed_floats(1) == 8 + sum(kp * c + c for kp, (_, c) in zip(k_padded, CHANNELS)) + 64 + 128 + 256 + 512 + 512
    assert lib.snerf_lpips_net_packed_floats(2) == 0 and lib.snerf_lpips_net_packed_floats(-1) == 0
    assert lib.snerf_lpips_net_workspace_bytes(1, 15, 64) == 0 and lib.snerf_lpips_net_workspace_bytes(1, 64, 15) == 0
    assert lib.snerf_lpips_net_workspace_bytes(1, 16, 16) > 0 and lib.snerf_lpips_net_workspace_bytes(2, 64, 64) == 0
    assert lib.snerf_lpips_net_workspace_bytes(1, 40000, 40000) == 0 and lib.snerf_lpips_net_workspace_bytes(1, 4200, 4200) == 0
    # five taps, two ping-pong regions (64 channels at full and 256 at quarter resolution), one pooled region, the partials
    floats = 2 * (756 * 1008 * (3 + 64 + 64) + 378 * 504 * (128 + 64) + 189 * 252 * (256 + 256) + 94 * 126 * 512 + 47 * 63 * 512)
    assert 4 * floats + 5 * 1024 * 8 <= lib.snerf_lpips_net_workspace_bytes(1, 756, 1008) <= 4 * floats + 5 * 1024 * 8 + 10 * 256
    assert ops.lpips_tap_shapes(756, 1008, net='vgg') == [(756, 1008, 64), (378, 504, 128), (189, 252, 256), (94, 126, 512), (47, 63, 512)]
    assert ops.lpips_tap_shapes(16, 16, net='vgg') == [(16, 16, 64), (8, 8, 128), (4, 4, 256), (2, 2, 512), (1, 1, 512)]
    # refused before anything is enqueued
    assert lib.snerf_lpips_net_sums(1, None, None, None, 64, 64, None, None, None, None, None) != 0
    assert b'lpips_sums: NULL pointer' in lib.snerf_last_error()
    assert lib.snerf_lpips_net_sums(3, None, None, None, 64, 64, None, None, None, None, None) != 0
    assert b'lpips_sums: network 3' in lib.snerf_last_error()
    assert lib.snerf_lpips_net_pack(1, None, None, None, None, None, None) != 0
    assert b'lpips_pack: NULL pointer' in lib.snerf_last_error()
    value = ctypes.c_int()
    with pytest.raises(RuntimeError, match='layer 5 outside'):
        _lib.check(lib.snerf_lpips_net_tap_shape(1, 64, 64, 5, ctypes.byref(value), ctypes.byref(value), ctypes.byref(value)), 'snerf_lpips_tap_shape')
    with pytest.raises(RuntimeError, match='a 15 x 64 image is smaller than the network.s 16 x 16'):
        _lib.check(lib.snerf_lpips_net_tap_shape(1, 15, 64, 0, ctypes.byref(value), ctypes.byref(value), ctypes.byref(value)), 'snerf_lpips_tap_shape')


def test_lpips_metrics_refuses_what_it_cannot_take():
    class Stub(torch.Tensor):
        """A host tensor that claims to live on the GPU: reaches the checks that follow the device check."""
        is_cuda = True

    def stub(shape, dtype=torch.uint8):
        return torch.zeros(shape, dtype=dtype).as_subclass(Stub)

    class Weights(qa.LpipsWeights):
        """VGG-16 weights without a device: what lpips_metrics looks at before it reaches the kernels."""

        def __init__(self):
            self.net = 'vgg'

    for shape in ((15, 64), (64, 15), (11, 11)):
        with pytest.raises(RuntimeError, match=f'gt_image: VGG-16 needs 16 pixels on every side, the image extent is {shape[0]} x {shape[1]}'):
            qa.lpips_metrics(stub(shape + (3,)), stub(shape + (3,)), Weights())
        with pytest.raises(RuntimeError, match=f'gt_image: VGG-16 needs 16 pixels on every side, the image extent is {shape[0]} x {shape[1]}'):
            ops.lpips_sums(stub(shape + (3,)), stub(shape + (3,)), None, net='vgg')
    with pytest.raises(RuntimeError, match=r'eval_image: expected shape \(64, 64, 3\), got \(64, 65, 3\)'):
        qa.lpips_metrics(stub((64, 65, 3)), stub((64, 64, 3)), Weights())
    with pytest.raises(RuntimeError, match="net: expected 'alex' or 'vgg', got 'squeeze'"):
        ops.lpips_sums(stub((64, 64, 3)), stub((64, 64, 3)), None, net='squeeze')
    with pytest.raises(RuntimeError, match="net: expected 'alex' or 'vgg', got 'squeeze'"):
        qa.LpipsWeights({}, 'cpu', net='squeeze')
    with pytest.raises(RuntimeError, match='lpips_pack: expected 13 convolution weights and biases and 5 lin weights'):
        ops.lpips_pack([None] * 5, [None] * 5, [None] * 5, net='vgg')
    with pytest.raises(RuntimeError, match=r'conv_weights\[2\]: expected shape \(128, 64, 3, 3\)'):
        ops.lpips_pack([stub((64, 3, 3, 3), torch.float32), stub((64, 64, 3, 3), torch.float32), stub((128, 64, 5, 5), torch.float32)] + [None] * 10,
                       [stub((64,), torch.float32), stub((64,), torch.float32)] + [None] * 11, [stub((1, 64, 1, 1), torch.float32)] + [None] * 4,
                       net='vgg')
    with pytest.raises(RuntimeError, match=r'lin_weights\[0\]: expected shape \(1, 64, 1, 1\) or \(64,\), got \(128,\)'):
        ops.lpips_pack([stub((64, 3, 3, 3), torch.float32), stub((64, 64, 3, 3), torch.float32)] + [None] * 11,
                       [stub((64,), torch.float32), stub((64,), torch.float32)] + [None] * 11, [stub((128,), torch.float32)] + [None] * 4, net='vgg')


def test_the_committed_tolerances_are_the_measured_ones():
    """The gates of tests/test_gpu_lpips_vgg.py are 4 x / 8 x the float32 restatement's distance from the float64 one, measured here
    with the committed restatement and inputs.  A CPU with another vector width may block the convolution's sums differently, so the
    fresh measurement has to reproduce the committed figure to a factor 1.5, not to the last bit."""
    measured = reference.precision_class()
    print(measured)
    assert test_gpu_lpips_vgg.SHAPES == reference.SHAPES
    assert test_gpu_lpips_vgg.FEATURE_TOLERANCE == 4 * test_gpu_lpips_vgg.FEATURE_MEASURED
    assert test_gpu_lpips_vgg.SUM_TOLERANCE == 8 * test_gpu_lpips_vgg.SUM_MEASURED
    assert test_gpu_lpips_vgg.SCORE_CAP == 5e-5
    assert test_gpu_lpips_vgg.FEATURE_MEASURED / 1.5 <= measured['feature'] <= test_gpu_lpips_vgg.FEATURE_MEASURED * 1.5
    assert test_gpu_lpips_vgg.SUM_MEASURED / 1.5 <= measured['sum'] <= test_gpu_lpips_vgg.SUM_MEASURED * 1.5
    # the cap sits far outside the measured gates; a 16-bit operand (2^-9 per product) would not pass the feature gate
    assert test_gpu_lpips_vgg.SUM_TOLERANCE * 0.03 < test_gpu_lpips_vgg.SCORE_CAP / 50 and measured['score'] < 1e-7
    assert test_gpu_lpips_vgg.FEATURE_TOLERANCE < 2.0 ** -9 / 100


def test_the_alexnet_fixture_is_what_its_generator_writes():
    golden = numpy.load(test_gpu_lpips_vgg.GOLDEN_ALEX)
    assert sorted(golden.files) == sorted(f'{kind}_{h}x{w}' for kind in ('plain', 'masked') for h, w in lpips_reference.SHAPES)
    weights = lpips_reference.random_weights()
    for h, w in lpips_reference.SHAPES:
        gt, image, mask = lpips_reference.random_images(h, w)
        for kind, m in (('plain', None), ('masked', mask)):
            recorded = golden[f'{kind}_{h}x{w}']
            assert recorded.dtype == numpy.float64 and recorded.shape == (5,)
            want = lpips_reference.lpips(gt, image, weights, mask=m)['sums']        # the float64 restatement, at the AlexNet test's gate
            assert max(abs(a - b) / abs(b) for a, b in zip(recorded, want)) <= 8 * 1.6480594426719216e-06
