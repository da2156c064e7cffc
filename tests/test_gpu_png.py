"""The PNG encoder on a real MI355X: ``ops.png_deflate`` on the smallest inputs at which each of its steps can go wrong, decoded by
tests/png_reference.py (chunk CRCs, zlib, un-filtering) and walked block by block against the contract of csrc/simplenerf_png.h,
then ``png_encoder='device'`` through the harness writers on the view sweep's and the validation pass's fixture models: the files of
the two routes decode to the same pixels."""
import ctypes
import os

import numpy
import pytest
import torch

from simplenerf_amd import _lib, harness, ops, synth
from simplenerf_amd.data_preprocessors.DataPreprocessor01 import DataPreprocessor
from simplenerf_amd.loss_functions.LossComputer01 import LossComputer
from simplenerf_amd.models.ModelFactory import get_model
from tests import png_reference as ref
from tests import util
from tests import validation_reference
from tests import view_sweep_reference

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def encode(images, mode=ops.PNG_FILTER_ADAPTIVE):
    """-> [stream bytes] of ``images`` (K,h,w[,3]) uint8 array through one ops.png_deflate call."""
    streams, sizes = ops.png_deflate(torch.from_numpy(numpy.ascontiguousarray(images)).to(DEV), mode)
    h, w = images.shape[1:3]
    channels = 3 if images.ndim == 4 else 1
    assert streams.shape == (len(images), _lib.load().snerf_png_deflate_bound_bytes(h, w, channels)) and streams.dtype == torch.uint8
    assert sizes.shape == (len(images),) and sizes.dtype == torch.int64
    streams, sizes = streams.cpu().numpy(), sizes.cpu().tolist()
    return [streams[i, :n].tobytes() for i, n in enumerate(sizes)]


def check(images, mode=ops.PNG_FILTER_ADAPTIVE):
    """Every property every case has: the CRCs verify, zlib accepts the stream, the length is exact, the pixels are equal, the size
    is within the bound, the rows carry the filter types of the rule (or ``mode``), the blocks are the contract's.
    -> [(stream, its strips' blocks)]"""
    results = []
    for image, stream in zip(images, encode(images, mode)):
        h, w = image.shape[:2]
        channels = 3 if image.ndim == 3 else 1
        assert len(stream) <= ref.bound_bytes(h, w, channels)
        pixels, kinds = ref.decode(ref.container(stream, h, w, channels))          # (raises on a CRC, zlib or length error)
        assert pixels.shape == image.shape and numpy.array_equal(pixels, image)
        assert kinds == ([mode] * h if mode >= 0 else ref.adaptive_kinds(image))
        results.append((stream, ref.check_contract(stream, ref.raw_bytes(h, w, channels))))
    return results


@pytest.mark.parametrize('pixel', [[[[7]]], [[[0]]], [[[[7, 8, 9]]]], [[[[0, 0, 0]]]]])
def test_one_pixel(pixel):
    (stream, strips), = check(numpy.array(pixel, dtype=numpy.uint8))
    assert len(strips) == 1


def test_noise_falls_back_to_stored_blocks():
    image = ref.noise(37, 53)
    (stream, strips), = check(image[None])
    assert [b['type'] for b in strips] == [0]
    assert len(ref.container(stream, 37, 53, 3)) <= 57 + ref.bound_bytes(37, 53, 3)          # (57 bytes of container)
    assert len(stream) == ref.raw_bytes(37, 53, 3) + 5 + 6


def test_smooth_frame_two_strips_cut_mid_row():
    image = ref.smooth(96, 128)
    assert ref.raw_bytes(96, 128, 3) == 36960 and 32768 % (1 + 128 * 3) != 0
    (stream, strips), = check(image[None])
    assert [b['type'] for b in strips] == [2, 2]
    device_file, host_file = ref.container(stream, 96, 128, 3), harness._png_bytes(image)
    print(f'96 x 128 x 3 smooth fixture: device encoder {len(device_file)} bytes, host writer {len(host_file)} bytes')
    assert len(device_file) < len(host_file)


@pytest.mark.parametrize('mode', [ops.PNG_FILTER_ADAPTIVE, 0])
@pytest.mark.parametrize('height', [64, 128])
def test_white_frames_long_runs_across_rows_and_the_cut(height, mode):
    """64 x 300: one strip of 19 264 bytes; 128 x 300: 38 528 bytes, so the runs also meet the cut between two strips."""
    (stream, strips), = check(numpy.full((1, height, 300), 255, dtype=numpy.uint8), mode)
    assert len(strips) == (1 if height == 64 else 2) and all(b['type'] == 2 for b in strips)
    assert max(length for b in strips for _, length, _ in b['matches']) == 258
    assert len(stream) < 400
    for block in strips:          # (check_contract: no match reaches back across the start of its strip)
        assert min(at for at, _, _ in block['matches']) > block['start']


def test_every_length_code_edge():
    (stream, strips), = check(ref.runs_row()[None], 0)
    assert tuple(length for _, length, _ in strips[0]['matches']) == ref.RUN_MATCHES


@pytest.mark.parametrize('chain', [False, True])
def test_fibonacci_counts_meet_the_15_bit_limit(chain):
    """The row of Fib(k + 1) counts for k = 0..20, and the row whose counts form the Fibonacci chain TOGETHER with the filter byte
    and the end-of-block symbol (png_reference.fibonacci_row): only the second has an unconstrained Huffman code deeper than 15."""
    row = ref.fibonacci_row(chain)
    assert row.shape == (1, 28654 if chain else 28656)
    (stream, strips), = check(row[None], 0)
    assert len(strips) == 1 and strips[0]['type'] == 2 and not strips[0]['matches']
    lengths = strips[0]['lengths']
    counts = numpy.bincount(numpy.concatenate([[0], row[0], [256]]))          # filter byte, pixels, end of block
    assert ref.huffman_depth(counts) == (20 if chain else 11)
    assert max(lengths) <= 15 and sum(1 for n in lengths if n) == (21 if chain else 22)
    assert len(stream) < 0.5 * row.size          # (the counts' entropy is 2.6 bits per byte)


def test_eight_frames_in_one_call_are_independent_and_repeatable():
    images = numpy.stack([ref.smooth(24, 32, seed=s) if s % 2 else ref.noise(24, 32, seed=s) // (1 + s) for s in range(8)])
    together = [stream for stream, _ in check(images)]
    assert len(set(together)) == 8
    for i in range(8):
        assert encode(images[i:i + 1])[0] == together[i], i
    assert encode(images) == together
    assert encode(images[::-1].copy()) == together[::-1]


@pytest.mark.parametrize('mode', range(5))
@pytest.mark.parametrize('channels', [3, 1])
def test_each_fixed_filter_type(mode, channels):
    check(ref.smooth(16, 20, channels, seed=5)[None], mode)


def test_bad_arguments_are_refused_with_a_message():
    good = torch.zeros((1, 4, 5, 3), dtype=torch.uint8, device=DEV)
    with pytest.raises(RuntimeError, match=r'snerf_png_deflate failed \(-1\).*filter_mode 7 outside -1..4'):
        ops.png_deflate(good, 7)
    with pytest.raises(RuntimeError, match=r'snerf_png_deflate failed \(-1\).*filter_mode -2'):
        ops.png_deflate(good, -2)
    with pytest.raises(RuntimeError, match=r'snerf_png_deflate failed \(-1\).*height 0'):
        ops.png_deflate(good[:, :0])
    with pytest.raises(RuntimeError, match='expected shape'):
        ops.png_deflate(torch.zeros((1, 4, 5, 4), dtype=torch.uint8, device=DEV))
    with pytest.raises(RuntimeError, match='expected uint8'):
        ops.png_deflate(good.float())
    lib = _lib.load()
    streams, sizes = ops.png_deflate(good)          # (sizes the workspace)
    work = ops._workspace('png', good.device, 1)
    null, stream = ctypes.c_void_p(0), ops._stream()
    arguments = dict(pixels=ops._ptr(good), images=1, height=4, width=5, channels=3, mode=-1, streams=ops._ptr(streams),
                     sizes=ops._ptr(sizes), work=ops._ptr(work))
    for change, word in (({'channels': 2}, 'channels 2'), ({'width': 0}, 'width 0'), ({'mode': 5}, 'filter_mode 5'), ({'images': -1}, 'images -1'),
                         ({'pixels': null}, 'NULL'), ({'streams': null}, 'NULL'), ({'sizes': null}, 'NULL'), ({'work': null}, 'NULL'),
                         ({'height': 65536, 'width': 32768, 'channels': 1}, '2^31')):
        status = lib.snerf_png_deflate(*{**arguments, **change}.values(), stream)
        assert status == _lib.C.SNERF_E_INVALID and word in lib.snerf_last_error().decode(), (change, status, lib.snerf_last_error())
    assert lib.snerf_png_deflate(null, 0, 4, 5, 3, -1, null, null, null, stream) == _lib.C.SNERF_OK
    empty_streams, empty_sizes = ops.png_deflate(good[:0])
    assert empty_streams.shape == (0, streams.shape[1]) and empty_sizes.shape == (0,)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ the harness writers
def decoded(path):
    with open(path, 'rb') as f:
        return ref.decode(f.read())


def files_under(directory):
    return sorted(os.path.relpath(os.path.join(root, name), directory) for root, _, names in os.walk(directory) for name in names)


def test_png_files_and_the_single_frame_writers(tmp_path):
    images = torch.from_numpy(numpy.stack([ref.smooth(37, 53, seed=s) for s in range(3)])).to(DEV)
    files = harness.png_files(images)
    assert len(files) == 3 and all(isinstance(f, bytes) for f in files)
    for i, blob in enumerate(files):
        assert numpy.array_equal(ref.decode(blob)[0], images[i].cpu().numpy())
    harness.save_image(tmp_path / 'host.png', images[0])
    harness.save_image(tmp_path / 'device.png', images[0], png_encoder='device')
    assert (tmp_path / 'device.png').read_bytes() == files[0] != (tmp_path / 'host.png').read_bytes()
    assert numpy.array_equal(decoded(tmp_path / 'device.png')[0], decoded(tmp_path / 'host.png')[0])
    depth = torch.from_numpy(numpy.random.RandomState(2).uniform(0, 9, (37, 53)).astype(numpy.float32)).to(DEV)
    for kind in ('host', 'device'):
        harness.save_depth(tmp_path / kind / 'a.png', depth, png_encoder=kind)
        harness.save_depth(tmp_path / kind / 'b.npy', depth, as_png=True, png_encoder=kind)
    assert files_under(tmp_path / 'device') == files_under(tmp_path / 'host') == ['a.png', 'b.npy', 'b.png']
    for name in ('a.png', 'b.png'):
        host_pixels, host_kinds = decoded(tmp_path / 'host' / name)
        device_pixels, device_kinds = decoded(tmp_path / 'device' / name)
        assert numpy.array_equal(host_pixels, device_pixels) and numpy.array_equal(host_pixels, validation_reference.preview_u8(depth.cpu().numpy()))
        assert host_kinds == [0] * 37 and device_kinds == ref.adaptive_kinds(host_pixels)
    assert (tmp_path / 'host' / 'b.npy').read_bytes() == (tmp_path / 'device' / 'b.npy').read_bytes()
    with pytest.raises(RuntimeError, match="png_encoder='device'"):
        harness.save_depth(tmp_path / 'c.png', depth.cpu(), png_encoder='device')


def test_static_camera_frames_of_the_two_encoders_decode_to_the_same_pixels(tmp_path):
    g, configs, saved, scene_configs = view_sweep_reference.load_case('ndc')
    model = get_model(synth.with_overrides(configs, hip_precision='fp32'), None)
    model.load_state_dict(util.golden_params(configs, g), strict=True)
    model = model.to(DEV).eval()
    dp = DataPreprocessor(scene_configs, 'test', model_configs=saved, device=DEV)
    extrinsics = numpy.concatenate([g['pose'][None], g['view_poses']])
    results = {kind: harness.save_static_camera_frames(model, model.configs, dp, extrinsics, tmp_path / kind, DEV, png_encoder=kind)
               for kind in ('host', 'device')}
    assert sorted(results['host']) == sorted(results['device'])
    names = [os.path.join('predicted_frames', f'{i:04}.png') for i in range(3)]
    assert files_under(tmp_path / 'host') == files_under(tmp_path / 'device') == names
    for i, name in enumerate(names):
        host_pixels, device_pixels = decoded(tmp_path / 'host' / name)[0], decoded(tmp_path / 'device' / name)[0]
        assert numpy.array_equal(host_pixels, device_pixels) and numpy.array_equal(device_pixels, results['device']['images'][i]), name


def test_run_validation_and_sample_images_of_the_two_encoders_decode_to_the_same_pixels(tmp_path):
    g, configs, train_raw, held_raw = validation_reference.load_prep('ndc')
    gp = util.load('validation_pass.npz')
    configs = synth.with_overrides(configs, hip_precision='fp32')
    model = get_model(configs, None)
    model.load_state_dict(validation_reference.pass_weights(configs, gp), strict=True)
    model = model.to(DEV).train()
    trained = DataPreprocessor(configs, 'train', train_raw, device=DEV)
    held = DataPreprocessor(configs, 'validation', held_raw, trained.get_model_configs(), device=DEV)
    losses = LossComputer(configs)
    totals, kept = {}, {}
    for kind in ('host', 'device'):
        kept[kind] = {}
        totals[kind] = harness.run_validation(model, losses, held, 41, configs, save_dirpath=tmp_path / kind, keep=kept[kind], png_encoder=kind)
        harness.save_sample_images(model, configs, [trained, held], 41, tmp_path / (kind + '_samples'), png_encoder=kind)
    assert totals['host'] == totals['device'] and sorted(kept['host']) == sorted(kept['device'])
    for directory in ('', '_samples'):
        names = files_under(tmp_path / ('host' + directory))
        assert names == files_under(tmp_path / ('device' + directory)) and any(name.endswith('.png') for name in names)
        colour = grey = 0
        for name in names:
            host_path, device_path = tmp_path / ('host' + directory) / name, tmp_path / ('device' + directory) / name
            if name.endswith('.npy'):
                assert host_path.read_bytes() == device_path.read_bytes(), name
                continue
            host_pixels, device_pixels = decoded(host_path)[0], decoded(device_path)[0]
            assert host_pixels.shape == device_pixels.shape and numpy.array_equal(host_pixels, device_pixels), name
            colour, grey = colour + (host_pixels.ndim == 3), grey + (host_pixels.ndim == 2)
        assert colour and grey
    for key, entry in kept['host'].items():
        assert numpy.array_equal(entry['u8'], kept['device'][key]['u8']), key
