"""The PNG encoder's host side: the decoder the GPU tests rely on (against a plain numpy filterer and a hand-written file), the
binding's fifth header group, the untouched default writer and the refusals of the ``png_encoder`` keyword -- none of it needs a GPU.
The coder's workgroup programs themselves run on the host in tests/test_png_coder_host.py."""
import os
import struct
import zlib

import numpy
import pytest
import torch

from simplenerf_amd import _lib, harness
from tests import png_reference as ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize('kind', range(5))
@pytest.mark.parametrize('shape', [(5, 7, 3), (5, 7)])
def test_decoder_inverts_each_filter_type(kind, shape):
    pixels = numpy.random.default_rng(10 * kind + len(shape)).integers(0, 256, size=shape, dtype=numpy.uint8)
    filtered = ref.filter_image(pixels, [kind] * shape[0])
    assert len(filtered) == ref.raw_bytes(shape[0], shape[1], 3 if len(shape) == 3 else 1)
    if kind:
        assert filtered != ref.filter_image(pixels, [0] * shape[0])
    decoded, kinds = ref.decode(ref.container(zlib.compress(filtered), shape[0], shape[1], 3 if len(shape) == 3 else 1))
    assert kinds == [kind] * shape[0] and decoded.shape == shape and numpy.array_equal(decoded, pixels)


def test_decoder_on_mixed_types_and_the_restated_rule():
    pixels = ref.smooth(6, 9, seed=3)
    decoded, kinds = ref.decode(ref.container(zlib.compress(ref.filter_image(pixels, [4, 3, 2, 1, 0, 4])), 6, 9, 3))
    assert kinds == [4, 3, 2, 1, 0, 4] and numpy.array_equal(decoded, pixels)
    # the rule: a flat row costs 0 with Sub and with None only if it is zeros; a tie goes to the lowest type
    flat = numpy.full((3, 8), 9, dtype=numpy.uint8)
    assert ref.adaptive_kinds(flat) == [1, 2, 2]          # row 0: Sub leaves one 9 (Paeth too: the lower type wins); then Up gives zeros
    assert ref.adaptive_kinds(numpy.zeros((2, 4, 3), dtype=numpy.uint8)) == [0, 0]
    ramp = numpy.arange(40, dtype=numpy.uint8).reshape(1, 40) * 3
    assert ref.adaptive_kinds(ramp) == [1]


def test_decoder_on_a_hand_written_paeth_file():
    """2 x 2 RGB, both rows of type 4.  Row 0 (above = zeros: Paeth predicts the left pixel): 10 20 30 | 13 19 35 -> 10 20 30, 3 255 5.
    Row 1: pixel (12 25 28): left 0, above (10 20 30), above-left 0 -> predicts above -> 2 5 254;  pixel (20 20 20): a = (12 25 28),
    b = (13 19 35), c = (10 20 30): p = a + b - c = (15 24 33); |p-a| = (3 1 5), |p-b| = (2 5 2), |p-c| = (5 4 3) -> b, a, b
    -> 20-13, 20-25, 20-35 = 7 251 241."""
    filtered = bytes([4, 10, 20, 30, 3, 255, 5,
                      4, 2, 5, 254, 7, 251, 241])
    stored = b'\x01' + struct.pack('<HH', len(filtered), len(filtered) ^ 0xFFFF) + filtered
    stream = b'\x78\x01' + stored + struct.pack('>I', zlib.adler32(filtered))
    ihdr = b'IHDR' + bytes([0, 0, 0, 2, 0, 0, 0, 2, 8, 2, 0, 0, 0])
    idat = b'IDAT' + stream
    blob = (b'\x89PNG\r\n\x1a\n' + struct.pack('>I', 13) + ihdr + struct.pack('>I', zlib.crc32(ihdr))
            + struct.pack('>I', len(stream)) + idat + struct.pack('>I', zlib.crc32(idat))
            + bytes([0, 0, 0, 0]) + b'IEND' + bytes([0xAE, 0x42, 0x60, 0x82]))
    pixels, kinds = ref.decode(blob)
    assert kinds == [4, 4]
    assert pixels.tolist() == [[[10, 20, 30], [13, 19, 35]], [[12, 25, 28], [20, 20, 20]]]
    with pytest.raises(ValueError, match='CRC'):
        ref.decode(blob[:40] + bytes([blob[40] ^ 1]) + blob[41:])


def test_bound_formula():
    assert ref.raw_bytes(96, 128, 3) == 36960 and ref.bound_bytes(96, 128, 3) == 36960 + 20 + 6
    assert ref.bound_bytes(1, 1, 1) == 2 + 10 + 6
    assert ref.bound_bytes(1, 32767, 1) == 32768 + 10 + 6 and ref.bound_bytes(1, 32768, 1) == 32769 + 20 + 6


def test_fixtures():
    assert ref.smooth(96, 128).shape == (96, 128, 3) and numpy.array_equal(ref.smooth(96, 128), ref.smooth(96, 128))
    row = ref.fibonacci_row()
    assert row.shape == (1, 28656) and numpy.bincount(row[0]).tolist()[:5] == [1, 1, 2, 3, 5] and numpy.bincount(row[0])[20] == 10946
    chain = ref.fibonacci_row(chain=True)
    assert chain.shape == (1, 28654) and numpy.bincount(chain[0]).tolist()[:4] == [0, 2, 3, 5] and numpy.bincount(chain[0])[19] == 10946
    assert ref.huffman_depth([1, 1] + numpy.bincount(chain[0]).tolist()) == 20 and ref.huffman_depth([1, 1, 1, 1]) == 2
    assert ref.runs_row().shape == (1, sum(ref.RUN_LENGTHS))


def test_png_headers_are_exactly_the_one_new_header():
    assert [os.path.relpath(path, REPO) for path in _lib.PNG_HEADERS] == [os.path.join('simplenerf_amd', 'csrc', 'simplenerf_png.h')]
    assert set(_lib.PNG_SIGNATURES) == {'snerf_png_deflate_bound_bytes', 'snerf_png_deflate_workspace_bytes', 'snerf_png_deflate'}
    earlier = set(_lib.SIGNATURES) | set(_lib.ADDED_SIGNATURES) | set(_lib.SWEEP_SIGNATURES) | set(_lib.SWEEP16_SIGNATURES)
    assert not earlier & set(_lib.PNG_SIGNATURES)
    import ctypes
    assert _lib.PNG_SIGNATURES['snerf_png_deflate_bound_bytes'] == (ctypes.c_size_t, [ctypes.c_int] * 3)
    restype, argtypes = _lib.PNG_SIGNATURES['snerf_png_deflate']
    assert restype is ctypes.c_int and argtypes == [ctypes.c_void_p] + [ctypes.c_int] * 5 + [ctypes.c_void_p] * 4
    assert _lib.C.SNERF_PNG_FILTER_ADAPTIVE == -1 and _lib.C.SNERF_PNG_STRIP_BYTES == ref.STRIP_BYTES
    assert _lib.ABI_VERSION == 10
    if os.path.exists(_lib.LIB_PATH):
        lib = _lib.load()
        for name in _lib.PNG_SIGNATURES:
            assert hasattr(lib, name), name
        # the queries are host code: the contract's bound, and 0 for what the call rejects
        for h, w, c in ((1, 1, 1), (96, 128, 3), (756, 1008, 3), (1, 32768, 1)):
            raw = ref.raw_bytes(h, w, c)
            assert raw + 6 < lib.snerf_png_deflate_bound_bytes(h, w, c) <= ref.bound_bytes(h, w, c)
            assert lib.snerf_png_deflate_workspace_bytes(2, h, w, c) >= 2 * raw
        assert lib.snerf_png_deflate_bound_bytes(4, 4, 2) == 0 and lib.snerf_png_deflate_bound_bytes(0, 4, 3) == 0
        assert lib.snerf_png_deflate_bound_bytes(65536, 32768, 1) == 0          # 2^31 bytes and more
        assert lib.snerf_png_deflate_workspace_bytes(0, 4, 4, 3) == 0


def test_default_writer_is_unchanged(tmp_path):
    image = ref.smooth(9, 13, seed=4)
    harness.save_image(tmp_path / 'a.png', image)
    harness.save_image(tmp_path / 'b.png', torch.from_numpy(image), png_encoder='host')
    rows = numpy.concatenate([numpy.zeros((9, 1), dtype=numpy.uint8), image.reshape(9, -1)], axis=1)
    expected = ref.container(zlib.compress(rows.tobytes(), 6), 9, 13, 3)
    assert (tmp_path / 'a.png').read_bytes() == (tmp_path / 'b.png').read_bytes() == harness._png_bytes(image) == expected
    pixels, kinds = ref.decode(expected)
    assert kinds == [0] * 9 and numpy.array_equal(pixels, image)
    depth = numpy.linspace(0, 4, 35, dtype=numpy.float32).reshape(5, 7)
    harness.save_depth(tmp_path / 'd.png', depth)
    assert (tmp_path / 'd.png').read_bytes() == harness._png_bytes(numpy.round(depth / depth.max() * 255).astype('uint8'))


def test_a_bad_png_encoder_raises_by_name(tmp_path):
    image = ref.smooth(4, 5)
    for call in (lambda: harness.save_image(tmp_path / 'a.png', image, png_encoder='gpu'),
                 lambda: harness.save_depth(tmp_path / 'b.png', image[:, :, 0].astype(numpy.float32), png_encoder='Device'),
                 lambda: harness._convert_and_write([], (4, 5), 0, None, None, png_encoder=None),
                 lambda: harness.save_static_camera_frames(None, {}, None, [], tmp_path, 'cpu', png_encoder='zlib'),
                 lambda: harness.save_sample_images(None, {}, [], 0, tmp_path, png_encoder=''),
                 lambda: harness.run_validation(None, None, None, 0, {}, png_encoder='hip')):
        with pytest.raises(RuntimeError, match="png_encoder: expected 'host' or 'device'"):
            call()
    assert not list(tmp_path.iterdir()) or all(p.is_dir() for p in tmp_path.iterdir())


def test_device_encoder_refuses_host_arrays(tmp_path):
    image = ref.smooth(4, 5)
    with pytest.raises(RuntimeError, match="png_encoder='device'.*ndarray.*no fall-back"):
        harness.save_image(tmp_path / 'a.png', image, png_encoder='device')
    with pytest.raises(RuntimeError, match="png_encoder='device'.*Tensor on cpu"):
        harness.save_image(tmp_path / 'a.png', torch.from_numpy(image), png_encoder='device')
    with pytest.raises(RuntimeError, match="png_encoder='device'"):
        harness.save_depth(tmp_path / 'b.npy', image[:, :, 0].astype(numpy.float32), as_png=True, png_encoder='device')
    with pytest.raises(RuntimeError, match="png_encoder='device'"):
        harness.png_files(image[None])
    assert not (tmp_path / 'a.png').exists() and not (tmp_path / 'b.npy').exists() and not (tmp_path / 'b.png').exists()
