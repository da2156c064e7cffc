"""Host side of LPIPS (qa.lpips_metrics, csrc/lpips.hip): the checkpoint loader, the restatement the metric is pinned to
(tests/lpips_reference.py), the index arithmetic of csrc/conv_index.h walked on the host under sanitizers, the exported symbols, the
refusals and the measured tolerance constants of tests/test_gpu_lpips.py -- none of it needs a GPU."""
import os
import subprocess

import numpy
import pytest
import torch

from simplenerf_amd import _lib, ops, qa
from tests import lpips_reference, test_gpu_lpips

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('snerf_lpips_packed_floats', 'snerf_lpips_pack', 'snerf_lpips_workspace_bytes', 'snerf_lpips_tap_shape', 'snerf_lpips_sums')
LPIPS_KEYS = ('net.slice1.0', 'net.slice2.3', 'net.slice3.6', 'net.slice4.8', 'net.slice5.10')
TORCHVISION_KEYS = ('features.0', 'features.3', 'features.6', 'features.8', 'features.10')


def checkpoints():
    """The same 15 tensors in both layouts, built here: (a saved lpips.LPIPS state dict, torchvision's AlexNet, alex.pth, tensors)."""
    tensors = lpips_reference.random_weights(5)
    package, torchvision, lin = {}, {}, {}
    for l in range(5):
        for part, group in (('weight', 'conv_weights'), ('bias', 'conv_biases')):
            package[f'{LPIPS_KEYS[l]}.{part}'] = tensors[group][l].clone()
            torchvision[f'{TORCHVISION_KEYS[l]}.{part}'] = tensors[group][l].clone()
        lin[f'lin{l}.model.1.weight'] = tensors['lin_weights'][l].reshape(1, -1, 1, 1).clone()
        package[f'lin{l}.model.1.weight'] = lin[f'lin{l}.model.1.weight'].clone()
        package[f'lins.{l}.model.1.weight'] = lin[f'lin{l}.model.1.weight'].clone()
    package['scaling_layer.shift'] = torch.tensor(lpips_reference.SHIFT).reshape(1, 3, 1, 1)
    package['scaling_layer.scale'] = torch.tensor(lpips_reference.SCALE).reshape(1, 3, 1, 1)
    torchvision['classifier.1.weight'] = torch.zeros(8, 8)          # ignored
    torchvision['classifier.1.bias'] = torch.zeros(8)
    return package, torchvision, lin, tensors


def same_tensors(got, want):
    return all(len(got[g]) == 5 and all(torch.equal(a, b) and a.dtype == torch.float32 for a, b in zip(got[g], want[g]))
               for g in ('conv_weights', 'conv_biases', 'lin_weights')) and all(torch.equal(got[k], want[k]) for k in ('shift', 'scale'))


def test_both_checkpoint_layouts_give_the_same_tensors(tmp_path):
    package, torchvision, lin, tensors = checkpoints()
    assert same_tensors(qa.lpips_tensors(package), tensors)
    assert same_tensors(qa.lpips_tensors(torchvision, lin), tensors)
    assert [tuple(t.shape) for t in qa.lpips_tensors(package)['lin_weights']] == [(64,), (192,), (384,), (256,), (256,)]
    # only the `lins.{k}` duplicates present; float64 tensors are converted
    renamed = {k: v.double() for k, v in package.items() if not k.startswith('lin')}
    renamed.update({k: v for k, v in package.items() if k.startswith('lins.')})
    assert same_tensors(qa.lpips_tensors(renamed), tensors)
    # the files are plain dictionaries of tensors: torch.load(weights_only=True) reads them back
    torch.save(torchvision, tmp_path / 'alexnet.pth')
    torch.save(lin, tmp_path / 'alex.pth')
    state = torch.load(tmp_path / 'alexnet.pth', map_location='cpu', weights_only=True)
    assert same_tensors(qa.lpips_tensors(state, torch.load(tmp_path / 'alex.pth', map_location='cpu', weights_only=True)), tensors)
    # scaling_layer.* overrides the constants
    package['scaling_layer.shift'] = torch.tensor([0.1, -0.2, 0.05]).reshape(1, 3, 1, 1)
    package['scaling_layer.scale'] = torch.tensor([0.5, 0.3, 0.4]).reshape(1, 3, 1, 1)
    got = qa.lpips_tensors(package)
    assert got['shift'].tolist() == torch.tensor([0.1, -0.2, 0.05]).tolist() and got['scale'].tolist() == torch.tensor([0.5, 0.3, 0.4]).tolist()
    assert qa.lpips_tensors(torchvision, lin)['shift'].tolist() == torch.tensor(qa.LPIPS_SHIFT).tolist()


def test_the_loader_names_what_is_wrong():
    package, torchvision, lin, _ = checkpoints()
    with pytest.raises(RuntimeError, match=r'lin0\.model\.1\.weight: missing'):
        qa.lpips_tensors(torchvision)                       # torchvision's file alone has no lin layers
    with pytest.raises(RuntimeError, match=r"neither .*net\.slice1\.0\.weight.*features\.0\.weight"):
        qa.lpips_tensors(lin)                               # alex.pth alone: an unknown layout
    with pytest.raises(RuntimeError, match=r"neither .*net\.slice1\.0\.weight"):
        qa.lpips_tensors({'module.features.0.weight': torch.zeros(64, 3, 11, 11)})
    with pytest.raises(RuntimeError, match='state_dict: expected a dictionary'):
        qa.lpips_tensors(torch.zeros(3))
    for key in ('features.6.bias', 'features.10.weight'):
        with pytest.raises(RuntimeError, match=key.replace('.', r'\.') + ': missing'):
            qa.lpips_tensors({k: v for k, v in torchvision.items() if k != key}, lin)
    with pytest.raises(RuntimeError, match=r'net\.slice4\.8\.weight: missing'):
        qa.lpips_tensors({k: v for k, v in package.items() if k != 'net.slice4.8.weight'})
    with pytest.raises(RuntimeError, match=r'lin3\.model\.1\.weight: missing'):
        qa.lpips_tensors(torchvision, {k: v for k, v in lin.items() if k != 'lin3.model.1.weight'})
    with pytest.raises(RuntimeError, match=r'features\.3\.weight: expected a tensor of shape \(192, 64, 5, 5\), got \(192, 64, 3, 3\)'):
        qa.lpips_tensors(dict(torchvision, **{'features.3.weight': torch.zeros(192, 64, 3, 3)}), lin)
    with pytest.raises(RuntimeError, match=r'features\.0\.bias: expected a tensor of shape \(64,\), got \(63,\)'):
        qa.lpips_tensors(dict(torchvision, **{'features.0.bias': torch.zeros(63)}), lin)
    with pytest.raises(RuntimeError, match=r'lin2\.model\.1\.weight: expected a tensor of shape \(1, 384, 1, 1\), got \(1, 256, 1, 1\)'):
        qa.lpips_tensors(torchvision, dict(lin, **{'lin2.model.1.weight': torch.zeros(1, 256, 1, 1)}))
    with pytest.raises(RuntimeError, match=r'scaling_layer\.scale: expected a tensor of 3 values'):
        qa.lpips_tensors(dict(package, **{'scaling_layer.scale': torch.ones(4)}))


def test_restatement_identical_images_and_masks():
    weights = lpips_reference.random_weights()
    gt, image, mask = lpips_reference.random_images(37, 53)
    for dtype in (torch.float64, torch.float32):
        assert lpips_reference.lpips(gt, gt, weights, dtype)['score'] == 0.0
        assert lpips_reference.lpips(gt, image, weights, dtype, mask=numpy.zeros((37, 53), dtype=bool))['score'] == 0.0
    plain = lpips_reference.lpips(gt, image, weights)
    assert lpips_reference.lpips(gt, image, weights, mask=numpy.ones((37, 53), dtype=bool))['score'] == plain['score']
    assert 0 < lpips_reference.lpips(gt, image, weights, mask=mask)['score'] < plain['score']
    assert [tuple(t.shape) for t in plain['taps']] == [(2, 64, 8, 12), (2, 192, 3, 5), (2, 384, 1, 2), (2, 256, 1, 2), (2, 256, 1, 2)]
    assert abs(sum(s / (t.shape[2] * t.shape[3]) for s, t in zip(plain['sums'], plain['taps'])) - plain['score']) < 1e-15
    # im2tensor: float32, in the package's order of operations
    frame = numpy.arange(256, dtype=numpy.uint8).repeat(3).reshape(16, 16, 3)
    want = (frame.astype(numpy.float32) * numpy.float32(2) / numpy.float32(255) - numpy.float32(1)).transpose(2, 0, 1)
    assert torch.equal(lpips_reference.im2tensor(frame)[0], torch.from_numpy(want)) and lpips_reference.im2tensor(frame).dtype == torch.float32


def test_restatement_on_a_hand_sized_case():
    """The first tap (scaling, conv k11 s4 p2 with bias, ReLU) and its layer score with explicit loops over the output pixels, the
    channels and the padded window, in float64: the restatement agrees to 1e-12."""
    weights = lpips_reference.random_weights(3)
    gt, image, _ = lpips_reference.random_images(31, 33, seed=9)
    got = lpips_reference.lpips(gt, image, weights)
    w = weights['conv_weights'][0].double().numpy()
    b = weights['conv_biases'][0].double().numpy()
    lin = weights['lin_weights'][0].double().numpy()
    shift, scale = weights['shift'].double().numpy(), weights['scale'].double().numpy()
    features = []
    for frame in (gt, image):
        x = (frame.astype(numpy.float32) * numpy.float32(2) / numpy.float32(255) - numpy.float32(1)).astype(numpy.float64)
        x = (x - shift) / scale                                         # (h, w, 3)
        out_h, out_w = (31 + 4 - 11) // 4 + 1, (33 + 4 - 11) // 4 + 1
        assert (out_h, out_w) == (7, 7)
        f = numpy.zeros((64, out_h, out_w))
        for oy in range(out_h):
            for ox in range(out_w):
                for n in range(64):
                    total = b[n]
                    for ky in range(11):
                        iy = oy * 4 - 2 + ky
                        if iy < 0 or iy >= 31:
                            continue                                    # zero padding
                        lo, hi = max(0, 2 - ox * 4), min(11, 33 + 2 - ox * 4)     # taps whose column lies inside the image
                        for c in range(3):
                            total += numpy.dot(w[n, c, ky, lo:hi], x[iy, ox * 4 - 2 + lo:ox * 4 - 2 + hi, c])
                    f[n, oy, ox] = max(total, 0.0)
        features.append(f)
    for k in range(2):
        assert numpy.abs(got['taps'][0][k].numpy() - features[k]).max() <= 1e-12 * numpy.abs(features[k]).max()
    total = 0.0
    for oy in range(7):
        for ox in range(7):
            a, e = features[0][:, oy, ox], features[1][:, oy, ox]
            a, e = a / (numpy.sqrt(numpy.sum(a * a)) + 1e-10), e / (numpy.sqrt(numpy.sum(e * e)) + 1e-10)
            total += numpy.sum(lin * (a - e) ** 2)
    assert abs(got['sums'][0] - total) <= 1e-12 * total and abs(got['layers'][0] - total / 49) <= 1e-12 * total / 49


def test_conv_index_walk_on_the_host_under_sanitizers(tmp_path):
    """tests/native/conv_index_test.cpp enumerates every (output pixel, k) of every layer through csrc/conv_index.h for the test
    shapes and a full 756 x 1008 frame, built with AddressSanitizer + UBSan, as its own process."""
    exe = str(tmp_path / 'conv_index_test')
    r = subprocess.run(['g++', '-O1', '-g', '-std=c++17', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                        os.path.join(REPO, 'tests', 'native', 'conv_index_test.cpp'), '-o', exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    shapes = lpips_reference.SHAPES + ((756, 1008),)
    r = subprocess.run([exe] + [str(v) for shape in shapes for v in shape], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, ASAN_OPTIONS='detect_leaks=0'))
    assert r.returncode == 0 and 'conv_index_test: OK' in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    assert 'extents 756 x 1008: 188 x 251 93 x 125 46 x 62 46 x 62 46 x 62' in r.stdout
    assert 'extents 31 x 31: 7 x 7 3 x 3 1 x 1 1 x 1 1 x 1' in r.stdout
    # the extents the test program derived are those of the restatement's taps
    weights = lpips_reference.random_weights()
    for h, w in lpips_reference.SHAPES:
        gt, image, _ = lpips_reference.random_images(h, w)
        want = ' '.join(f'{t.shape[2]} x {t.shape[3]}' for t in lpips_reference.taps(lpips_reference.im2tensor(gt), weights, torch.float32))
        assert f'extents {h} x {w}: {want}\n' in r.stdout
    r = subprocess.run([exe, '30', '64'], capture_output=True, text=True, timeout=60, env=dict(os.environ, ASAN_OPTIONS='detect_leaks=0'))
    assert r.returncode == 1 and 'FAILED' in r.stdout


def test_library_exports_the_lpips_entry_points():
    header = open(os.path.join(REPO, 'include', 'simplenerf_hip.h')).read()
    lib = _lib.load()
    for name in NAMES:
        assert name + '(' in header and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert lib.snerf_abi_version() == _lib.ABI_VERSION == 10
    # shift, scale, padding | W[k_padded][c_out] + bias per layer | the lin layers
    k_padded = [-(-(c_in * k * k) // 32) * 32 for _, c_in, k in ops.LPIPS_CONVS]
    assert k_padded == [384, 1600, 1728, 3456, 2304]
    assert lib.snerf_lpips_packed_floats() == 8 + sum(kp * c + c for kp, (c, _, _) in zip(k_padded, ops.LPIPS_CONVS)) + sum(c for c, _, _ in ops.LPIPS_CONVS)
    assert lib.snerf_lpips_workspace_bytes(30, 64) == 0 and lib.snerf_lpips_workspace_bytes(64, 30) == 0
    assert lib.snerf_lpips_workspace_bytes(40000, 40000) == 0
    floats = 2 * (756 * 1008 * 3 + 188 * 251 * 64 + 93 * 125 * 64 + 93 * 125 * 192 + 46 * 62 * (192 + 384 + 256 + 256))
    assert 4 * floats + 5 * 1024 * 8 <= lib.snerf_lpips_workspace_bytes(756, 1008) <= 4 * floats + 5 * 1024 * 8 + 10 * 256
    assert ops.lpips_tap_shapes(756, 1008) == [(188, 251, 64), (93, 125, 192), (46, 62, 384), (46, 62, 256), (46, 62, 256)]
    assert ops.lpips_tap_shapes(31, 31) == [(7, 7, 64), (3, 3, 192), (1, 1, 384), (1, 1, 256), (1, 1, 256)]
    # refused before anything is enqueued
    assert lib.snerf_lpips_sums(None, None, None, 64, 64, None, None, None, None, None) != 0
    assert b'lpips_sums: NULL pointer' in lib.snerf_last_error()
    assert lib.snerf_lpips_pack(None, None, None, None, None, None) != 0
    assert b'lpips_pack: NULL pointer' in lib.snerf_last_error()
    with pytest.raises(RuntimeError, match='layer 5 outside'):
        import ctypes
        value = ctypes.c_int()
        _lib.check(lib.snerf_lpips_tap_shape(64, 64, 5, ctypes.byref(value), ctypes.byref(value), ctypes.byref(value)), 'snerf_lpips_tap_shape')


def test_lpips_metrics_refuses_what_it_cannot_take():
    class Stub(torch.Tensor):
        """A host tensor that claims to live on the GPU: reaches the checks that follow the device check."""
        is_cuda = True

    def stub(shape, dtype=torch.uint8):
        return torch.zeros(shape, dtype=dtype).as_subclass(Stub)

    with pytest.raises(RuntimeError, match='gt_image: expected a tensor on the GPU'):
        qa.lpips_metrics(stub((64, 64, 3)), torch.zeros((64, 64, 3), dtype=torch.uint8), None)
    with pytest.raises(RuntimeError, match='eval_image: expected uint8, got torch.float32'):
        qa.lpips_metrics(stub((64, 64, 3), torch.float32), stub((64, 64, 3)), None)
    with pytest.raises(RuntimeError, match=r'eval_image: expected shape \(64, 64, 3\), got \(64, 65, 3\)'):
        qa.lpips_metrics(stub((64, 65, 3)), stub((64, 64, 3)), None)
    with pytest.raises(RuntimeError, match=r'mask: expected shape \(64, 64\), got \(64, 64, 3\)'):
        qa.lpips_metrics(stub((64, 64, 3)), stub((64, 64, 3)), None, stub((64, 64, 3), torch.bool))
    for shape in ((30, 64), (64, 30), (11, 11)):
        with pytest.raises(RuntimeError, match=f'gt_image: AlexNet needs 31 pixels on every side, the image extent is {shape[0]} x {shape[1]}'):
            qa.lpips_metrics(stub(shape + (3,)), stub(shape + (3,)), None)
        with pytest.raises(RuntimeError, match=f'the image extent is {shape[0]} x {shape[1]}'):
            ops.lpips_sums(stub(shape + (3,)), stub(shape + (3,)), None)
    with pytest.raises(RuntimeError, match='weights: expected qa.LpipsWeights, got dict'):
        qa.lpips_metrics(stub((64, 64, 3)), stub((64, 64, 3)), {})
    with pytest.raises(RuntimeError, match=r'conv_weights\[1\]: expected shape \(192, 64, 5, 5\)'):
        ops.lpips_pack([stub((64, 3, 11, 11), torch.float32), stub((192, 64, 3, 3), torch.float32)] + [None] * 3,
                       [stub((64,), torch.float32)] + [None] * 4, [stub((1, 64, 1, 1), torch.float32)] + [None] * 4)
    with pytest.raises(RuntimeError, match=r'conv_weights\[0\]: expected a tensor on the GPU'):
        ops.lpips_pack([torch.zeros(64, 3, 11, 11)] + [None] * 4, [None] * 5, [None] * 5)


def test_summarise_takes_the_new_columns():
    rows = [{'frame_num': 3, 'PSNR': 20.123456, 'LPIPS': 0.123449}, {'frame_num': 4, 'PSNR': 21.0, 'LPIPS': 0.2, 'MaskedLPIPS': 0.05555}]
    table = qa.summarise(rows)
    assert table['frames'][0] == {'frame_num': 3, 'PSNR': 20.1235, 'LPIPS': 0.1234}
    assert table['average'] == {'PSNR': 20.5618, 'LPIPS': 0.1617, 'MaskedLPIPS': 0.0556}


def test_the_committed_tolerances_are_the_measured_ones():
    """The gates of tests/test_gpu_lpips.py are 4 x / 8 x the float32 restatement's distance from the float64 one, measured here with
    the committed restatement and inputs.  A CPU with another vector width may block the convolution's sums differently, so the
    fresh measurement has to reproduce the committed figure to a factor 1.5, not to the last bit."""
    measured = lpips_reference.precision_class()
    print(measured)
    assert test_gpu_lpips.SHAPES == lpips_reference.SHAPES == ((31, 31), (37, 53), (64, 80), (96, 131))
    assert test_gpu_lpips.FEATURE_TOLERANCE == 4 * test_gpu_lpips.FEATURE_MEASURED
    assert test_gpu_lpips.SUM_TOLERANCE == 8 * test_gpu_lpips.SUM_MEASURED
    assert test_gpu_lpips.SCORE_CAP == 5e-5
    assert test_gpu_lpips.FEATURE_MEASURED / 1.5 <= measured['feature'] <= test_gpu_lpips.FEATURE_MEASURED * 1.5
    assert test_gpu_lpips.SUM_MEASURED / 1.5 <= measured['sum'] <= test_gpu_lpips.SUM_MEASURED * 1.5
    # the cap sits far outside the measured gates; a 16-bit operand (2^-9 per product) would not pass the feature gate
    assert test_gpu_lpips.SUM_TOLERANCE * 0.03 < test_gpu_lpips.SCORE_CAP / 50 and measured['score'] < 1e-7
    assert test_gpu_lpips.FEATURE_TOLERANCE < 2.0 ** -9 / 100
