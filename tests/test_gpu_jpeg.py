"""The JPEG encoder on a real MI355X: ``ops.jpeg_scan`` must give, byte for byte, what the restated encoder of
tests/jpeg_reference.py gives (tests/test_jpeg_host.py holds that one to PIL) on the smallest inputs at which each of its steps can
go wrong -- one MCU with replication both ways, sizes that are no multiple of the MCU, ten MCU rows (RSTn wraps past D7), the longest
row of the workload as noise at quality 100 (two emit passes, stuffed FF bytes, the bound), the largest DC and AC categories, a block
whose 63rd coefficient alone is non-zero (three ZRL, no EOB), exactly one full emit pass and one block more, several transform chunks,
the qualities 1, 50, 90 and 100 -- then batches, the two host bindings, the refusals, and the video writers of the harness."""
import ctypes
import os

import numpy
import pytest
import torch

from simplenerf_amd import _lib, harness, ops, synth
from simplenerf_amd.data_preprocessors.DataPreprocessor01 import DataPreprocessor
from simplenerf_amd.models.ModelFactory import get_model
from tests import jpeg_reference as ref
from tests import util
from tests import view_sweep_reference

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def encode(images, quality, binding='ctypes'):
    """-> [scan bytes] of ``images`` (K,h,w[,3]) uint8 array through one ops.jpeg_scan call."""
    scans, sizes = ops.jpeg_scan(torch.from_numpy(numpy.ascontiguousarray(images)).to(DEV), quality, binding=binding)
    h, w = images.shape[1:3]
    channels = 3 if images.ndim == 4 else 1
    assert scans.shape == (len(images), _lib.load().snerf_jpeg_scan_bound_bytes(h, w, channels)) and scans.dtype == torch.uint8
    assert sizes.shape == (len(images),) and sizes.dtype == torch.int64
    scans, sizes = scans.cpu().numpy(), sizes.cpu().tolist()
    return [scans[i, :n].tobytes() for i, n in enumerate(sizes)]


@pytest.mark.parametrize('name', list(ref.CASES))
def test_device_bytes_equal_the_restated_encoder(name):
    image, quality, scan, symbols = ref.expected(name)
    produced, = encode(image[None], quality)
    assert len(produced) <= ref.bound_bytes(image.shape[0], image.shape[1], 3 if image.ndim == 3 else 1)
    assert produced == scan
    if name == '16x1008 colour noise':
        assert b'\xff\x00' in scan and ref.geometry(16, 1008, 3)[3] == 378          # a stuffed byte; two passes of the emit program
    if name.startswith('checkerboard'):
        assert max(size for kind, size in symbols if kind == 'dc') == 11 and max(s & 15 for kind, s in symbols if kind == 'ac') == 10
    if name == 'basis patterns':
        assert symbols[:6] == [('dc', 0), ('ac', 0xF0), ('ac', 0xF0), ('ac', 0xF0), ('ac', 14 << 4 | 3), ('dc', 0)]
    if name == '147x40 colour':
        h, w = image.shape[:2]
        assert ref.parse(ref.jfif(produced, h, w, 3, quality))['restart_markers'] == [0, 1, 2, 3, 4, 5, 6, 7, 0]


def test_three_frames_in_one_call_are_independent_and_repeatable():
    images = numpy.stack([ref.textured(37, 53, seed=1), ref.noise(37, 53), ref.checkerboard(37, 53, 3)])
    expected = [ref.scan(image, 75) for image in images]
    together = encode(images, 75)
    assert together == expected and len(set(together)) == 3
    for i in range(3):
        assert encode(images[i:i + 1], 75)[0] == together[i], i
    assert encode(images, 75) == together
    assert encode(images[::-1].copy(), 75) == together[::-1]
    grey = images[:, :, :, 1].copy()
    assert encode(grey, 75) == [ref.scan(image, 75) for image in grey]


def test_both_bindings_give_the_same_bytes():
    images = numpy.stack([ref.textured(19, 35, seed=s) for s in range(2)])
    for frames, quality in ((images, 90), (images[:, :, :, 0].copy(), 35)):
        through_ctypes, through_torch = encode(frames, quality), encode(frames, quality, binding='torch_ext')
        assert through_ctypes == through_torch == [ref.scan(image, quality) for image in frames]
    empty = torch.zeros((0, 4, 5, 3), dtype=torch.uint8, device=DEV)
    for binding in ops.JPEG_BINDINGS:
        scans, sizes = ops.jpeg_scan(empty, 90, binding=binding)
        assert scans.shape == (0, ref.bound_bytes(4, 5, 3)) and sizes.shape == (0,)
        with pytest.raises(RuntimeError, match=r'snerf_jpeg_scan failed \(-1\).*quality 101 outside 1..100'):
            ops.jpeg_scan(torch.zeros((1, 4, 5), dtype=torch.uint8, device=DEV), 101, binding=binding)
        with pytest.raises(RuntimeError, match='expected shape'):
            ops.jpeg_scan(torch.zeros((1, 4, 5, 4), dtype=torch.uint8, device=DEV), 90, binding=binding)
        with pytest.raises(RuntimeError, match='expected uint8'):
            ops.jpeg_scan(torch.zeros((1, 4, 5, 3), device=DEV), 90, binding=binding)


def test_bad_arguments_are_refused_with_a_message():
    good = torch.zeros((1, 4, 5, 3), dtype=torch.uint8, device=DEV)
    with pytest.raises(RuntimeError, match=r'snerf_jpeg_scan failed \(-1\).*quality 0 outside 1..100'):
        ops.jpeg_scan(good, 0)
    with pytest.raises(RuntimeError, match=r'snerf_jpeg_scan failed \(-1\).*height 0'):
        ops.jpeg_scan(good[:, :0])
    lib = _lib.load()
    scans, sizes = ops.jpeg_scan(good)          # (sizes the workspace)
    work = ops._workspace('jpeg', good.device, 1)
    null, stream = ctypes.c_void_p(0), ops._stream()
    arguments = dict(pixels=ops._ptr(good), images=1, height=4, width=5, channels=3, quality=90, scans=ops._ptr(scans),
                     sizes=ops._ptr(sizes), work=ops._ptr(work))
    odd = lambda pointer, by: ctypes.c_void_p(pointer.value + by)
    for change, word in (({'channels': 2}, 'channels 2'), ({'channels': 4}, 'channels 4'), ({'width': 0}, 'width 0'), ({'height': 65536}, 'height 65536'),
                         ({'width': 65536}, 'width 65536'), ({'quality': 0}, 'quality 0'), ({'quality': 101}, 'quality 101'),
                         ({'images': -1}, 'images -1'), ({'pixels': null}, 'NULL'), ({'scans': null}, 'NULL'), ({'sizes': null}, 'NULL'),
                         ({'work': null}, 'NULL'), ({'work': odd(ops._ptr(work), 8)}, '16-byte aligned'),
                         ({'sizes': odd(ops._ptr(sizes), 4)}, '8-byte aligned')):
        status = lib.snerf_jpeg_scan(*{**arguments, **change}.values(), stream)
        assert status == _lib.C.SNERF_E_INVALID and word in lib.snerf_last_error().decode(), (change, status, lib.snerf_last_error())
    # 2^31 - 1 frames of two MCU rows are 2^32 - 2 workgroups: refused before anything is enqueued
    status = lib.snerf_jpeg_scan(*{**arguments, 'images': 2 ** 31 - 1, 'height': 17}.values(), stream)
    assert status == _lib.C.SNERF_E_UNSUPPORTED and '2^31' in lib.snerf_last_error().decode()
    assert lib.snerf_jpeg_scan(null, 0, 4, 5, 3, 90, null, null, null, stream) == _lib.C.SNERF_OK
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ the harness writers
def test_jpeg_files_and_save_video_end_to_end(tmp_path, monkeypatch):
    images = numpy.stack([ref.textured(33, 17, seed=s) for s in range(4)])
    frames = torch.from_numpy(images).to(DEV)
    files = harness.jpeg_files(frames)
    assert files == [ref.encode(image, 90) for image in images]
    path = tmp_path / 'deep' / 'video.avi'
    harness.save_video(path, frames)
    walked = ref.walk_avi(path.read_bytes())
    assert walked['frames'] == files
    micro, _, _, _, count, _, _, _, width, height = walked['avih'][:10]
    assert (micro, count, width, height) == (66667, 4, 17, 33) and walked['strh'][6:8] == (1, 15)
    for data, image in zip(walked['frames'], images):
        assert data[:2] == b'\xff\xd8' and data[-2:] == b'\xff\xd9'
        decoded = ref.decode(data)
        assert decoded.shape == image.shape and numpy.array_equal(decoded, ref.decode(ref.encode(image, 90)))
    before = path.read_bytes()
    harness.save_video(path, frames[:1], quality=10)          # an existing file is left alone
    assert path.read_bytes() == before
    grey = tmp_path / 'grey.avi'
    harness.save_video(grey, frames[:2, :, :, 0].contiguous(), frame_rate=30, quality=50)
    walked = ref.walk_avi(grey.read_bytes())
    assert walked['frames'] == [ref.encode(image[:, :, 0], 50) for image in images[:2]] and walked['avih'][0] == 33333

    class TwoGiB(bytes):
        def __len__(self):
            return 1 << 31
    monkeypatch.setattr(harness, '_avi_bytes', lambda *args: TwoGiB())
    with pytest.raises(RuntimeError, match=r'huge\.avi would be 2147483648 bytes'):
        harness.save_video(tmp_path / 'huge.avi', frames)
    assert not (tmp_path / 'huge.avi').exists()


@pytest.mark.parametrize('precision', ['fp32', 'f16x3'])
def test_static_camera_and_camera_path_videos(precision, tmp_path):
    """'fp32' takes the one-trunk-pass route of the sweep, 'f16x3' the plain loop."""
    g, configs, saved, scene_configs = view_sweep_reference.load_case('ndc')
    configs = synth.with_overrides(configs, hip_precision=precision)
    model = get_model(configs, None)
    # seeded weights with the density head scaled up and centred on sigma = 0.5 (the plain initialisation is almost transparent)
    weights = synth.synth_state_dict(util.model_param_shapes(configs), 77, sigma_gain=60.0)
    for level in ('coarse', 'fine'):
        weights[f'{level}_model.pts_output_linear.bias'][0] = 0.5
    model.load_state_dict({k: torch.from_numpy(v) for k, v in weights.items()}, strict=True)
    model = model.to(DEV).eval()
    assert harness.view_sweep_is_fast(model) is (precision == 'fp32')
    dp = DataPreprocessor(scene_configs, 'test', model_configs=saved, device=DEV)
    extrinsics = numpy.concatenate([g['pose'][None], g['view_poses']])          # (4,4,4) raw poses
    cameras = [dp.camera(pose) for pose in extrinsics]

    def files_under(directory):
        return sorted(os.path.relpath(os.path.join(root, name), directory) for root, _, names in os.walk(directory) for name in names)

    result = harness.save_static_camera_video(model, model.configs, dp, extrinsics, tmp_path / 'static', DEV)
    assert files_under(tmp_path / 'static') == ['StaticCameraVideo.avi']          # no PNG frames
    swept = harness.predict_view_sweep(model, model.configs, cameras[0], cameras[1:], DEV, keep_device_images=True)
    assert numpy.array_equal(result['images'], swept['images']) and 'images_device' not in result
    walked = ref.walk_avi((tmp_path / 'static' / 'StaticCameraVideo.avi').read_bytes())
    assert len(walked['frames']) == len(extrinsics) - 1 == 3 and walked['avih'][8:10] == (11, 7)
    assert walked['frames'] == harness.jpeg_files(swept['images_device'])
    assert walked['frames'] == [ref.encode(image, 90) for image in swept['images']]

    harness.save_static_camera_video(model, model.configs, dp, extrinsics, tmp_path / 'picked', DEV, video_frame_nums=[2, 0, 0], quality=60)
    walked = ref.walk_avi((tmp_path / 'picked' / 'StaticCameraVideo.avi').read_bytes())
    assert walked['frames'] == harness.jpeg_files(swept['images_device'][[2, 0, 0]], 60)

    result = harness.save_camera_path_video(model, model.configs, dp, extrinsics, tmp_path / 'path', DEV)
    assert files_under(tmp_path / 'path') == ['PredictedVideo.avi']
    predicted = numpy.stack([harness.predict_frame(model, model.configs, camera, DEV)['image'] for camera in cameras[1:]])
    assert numpy.array_equal(result['images_device'].cpu().numpy(), predicted)
    walked = ref.walk_avi((tmp_path / 'path' / 'PredictedVideo.avi').read_bytes())
    assert len(walked['frames']) == len(extrinsics) - 1 and walked['avih'][8:10] == (11, 7)
    assert walked['frames'] == harness.jpeg_files(torch.from_numpy(predicted).to(DEV))
    assert len(set(walked['frames'])) == 3          # three poses, three different frames
    harness.save_camera_path_video(model, model.configs, dp, extrinsics, tmp_path / 'path_picked', DEV, video_frame_nums=numpy.array([1, 2]))
    walked = ref.walk_avi((tmp_path / 'path_picked' / 'PredictedVideo.avi').read_bytes())
    assert walked['frames'] == harness.jpeg_files(torch.from_numpy(predicted[[1, 2]]).to(DEV))
