"""The JPEG encoder's host side, without a GPU: the binding's sixth header group; the restated encoder of tests/jpeg_reference.py
(what the GPU tests hold the device to, byte for byte) judged by PIL -- its files open, and their quality and size are PIL's own --
and by the project's own decoder; the markers ``harness`` writes around a scan; the AVI container; frame selection.

Measured here with the restated encoder against PIL 12.2 (``quality`` 50 and 90, ``subsampling=2, optimize=False``) on six 96 x 128
fixtures -- png_reference.smooth (the PNG tests' smooth frame), jpeg_reference.textured, jpeg_reference.noise, each in colour and grey:
  PSNR of PIL's decode against the source, PIL's own file minus ours: -0.0053 .. +0.0116 dB (largest: smooth grey, quality 90).
      Gate: twice the largest shortfall, 0.0232 dB -- only the rounding of the DCT and colour steps differs.
  Bytes, (ours - structure - PIL's) / PIL's: -0.0213 .. -0.0039.  `structure` is what our layout carries and PIL's does not, stated
      apart from the measurement: the 6-byte DRI segment, and per MCU row 2 marker bytes (but the last), up to 1 byte of padding and
      the DC predictors' reset -- at most 20 bits for luminance (a 9-bit code and 11 bits) and 22 for each chrominance component,
      3 bytes grey and 8 colour.  No fixture is larger than PIL's file once that is taken off, so twice the largest excess is no
      excess: the gate is 0.
  Quantised levels that differ from round(float64 DCT / q), grey fixtures: ours 0.14 % .. 1.26 %, PIL's (read from its file by the
      project's decoder) 0.11 % .. 1.03 %; ours minus PIL's: +0.0003 .. +0.0024 (largest: noise, quality 90).  Gate: twice that, 0.0048.
The same figures are in profiles/jpeg_encode.json."""
import ctypes
import io
import os

import numpy
import pytest
import torch

from simplenerf_amd import _lib, harness, ops
from tests import jpeg_reference as ref
from tests import png_reference

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PSNR_SHORTFALL_DB = 2 * 0.0116
SIZE_EXCESS = 0.0
LEVEL_SHARE_EXCESS = 2 * 0.0024


def test_jpeg_headers_are_exactly_the_one_new_header():
    assert [os.path.relpath(path, REPO) for path in _lib.JPEG_HEADERS] == [os.path.join('simplenerf_amd', 'csrc', 'simplenerf_jpeg.h')]
    assert set(_lib.JPEG_SIGNATURES) == {'snerf_jpeg_scan_bound_bytes', 'snerf_jpeg_scan_workspace_bytes', 'snerf_jpeg_scan'}
    earlier = (set(_lib.SIGNATURES) | set(_lib.ADDED_SIGNATURES) | set(_lib.SWEEP_SIGNATURES) | set(_lib.SWEEP16_SIGNATURES)
               | set(_lib.PNG_SIGNATURES))
    assert not earlier & set(_lib.JPEG_SIGNATURES)
    assert _lib.JPEG_SIGNATURES['snerf_jpeg_scan_bound_bytes'] == (ctypes.c_size_t, [ctypes.c_int] * 3)
    assert _lib.JPEG_SIGNATURES['snerf_jpeg_scan_workspace_bytes'] == (ctypes.c_size_t, [ctypes.c_int] * 4)
    restype, argtypes = _lib.JPEG_SIGNATURES['snerf_jpeg_scan']
    assert restype is ctypes.c_int and argtypes == [ctypes.c_void_p] + [ctypes.c_int] * 5 + [ctypes.c_void_p] * 4
    assert _lib.C.SNERF_JPEG_BLOCK_BYTES == ref.BLOCK_BYTES and 8 * ref.BLOCK_BYTES >= 22 + 63 * 26
    assert _lib.ABI_VERSION == 10
    lib = _lib.load()          # (AttributeError if the library does not export a declared symbol)
    for name in _lib.JPEG_SIGNATURES:
        assert hasattr(lib, name), name
    # the queries are host code: the contract's bound, and 0 for each argument the call rejects
    for h, w, c in ((1, 1, 1), (1, 1, 3), (96, 128, 3), (756, 1008, 3), (65535, 65535, 1), (65535, 65535, 3)):
        assert lib.snerf_jpeg_scan_bound_bytes(h, w, c) == ref.bound_bytes(h, w, c)
    assert lib.snerf_jpeg_scan_bound_bytes(756, 1008, 3) == 48 * (2 * 208 * 63 * 6 + 2)
    blocks = 48 * 63 * 6
    assert lib.snerf_jpeg_scan_workspace_bytes(2, 756, 1008, 3) >= 2 * (blocks * 128 + ref.bound_bytes(756, 1008, 3))
    for h, w, c in ((4, 4, 2), (4, 4, 0), (4, 4, 4), (0, 4, 3), (4, 0, 3), (-1, 4, 1), (65536, 4, 1), (4, 65536, 3)):
        assert lib.snerf_jpeg_scan_bound_bytes(h, w, c) == 0, (h, w, c)
        assert lib.snerf_jpeg_scan_workspace_bytes(1, h, w, c) == 0, (h, w, c)
    assert lib.snerf_jpeg_scan_workspace_bytes(0, 4, 4, 3) == 0 and lib.snerf_jpeg_scan_workspace_bytes(-1, 4, 4, 3) == 0
    assert lib.snerf_jpeg_scan_workspace_bytes(2 ** 31 - 1, 16, 16, 1) == 0          # 2^32 workgroups: the call answers UNSUPPORTED


def test_the_restated_tables_are_the_standards_and_the_matrix_is_the_rounded_cosine():
    u, x = numpy.meshgrid(numpy.arange(8), numpy.arange(8), indexing='ij')
    exact = 8192 * numpy.where(u == 0, numpy.sqrt(1 / 8), 0.5) * numpy.cos((2 * x + 1) * u * numpy.pi / 16)
    assert numpy.array_equal(ref.DCT, numpy.rint(exact).astype(numpy.int64))
    assert sorted(ref.ZIGZAG.tolist()) == list(range(64)) and ref.ZIGZAG[:6].tolist() == [0, 1, 8, 16, 9, 2] and ref.ZIGZAG[63] == 63
    for key, (bits, values) in ref.HUFFMAN.items():
        assert sum(bits) == len(values) == len(set(values)) == (162 if key & 0x10 else 12)
        codes = ref.huffman_codes(bits, values)
        assert max(length for _, length in codes.values()) == {0x00: 9, 0x01: 11, 0x10: 16, 0x11: 16}[key]
        assert all(code != (1 << length) - 1 for code, length in codes.values())          # no code of 1-bits alone
    assert ref.quantisers(50)[0].tolist() == list(ref.QUANT_BASE[0]) and ref.quantisers(100).max() == 1
    assert ref.quantisers(1)[0].min() == 255 and ref.quantisers(90)[0, 0] == 3 and ref.quantisers(25)[1, 0] == 34
    # PIL writes the same tables at the same quality
    from PIL import Image
    for quality in (1, 25, 50, 90, 100):
        blob = io.BytesIO()
        Image.new('RGB', (16, 16)).save(blob, 'JPEG', quality=quality, subsampling=2, optimize=False)
        parsed = ref.parse(blob.getvalue())
        assert numpy.array_equal(parsed['quant'][0], ref.quantisers(quality)[0]) and numpy.array_equal(parsed['quant'][1], ref.quantisers(quality)[1])


@pytest.mark.parametrize('name', list(ref.CASES))
def test_restated_files_open_in_pil_and_decode_to_the_levels_that_were_coded(name):
    from PIL import Image
    image, quality, scan, symbols = ref.expected(name)
    h, w = image.shape[:2]
    channels = 3 if image.ndim == 3 else 1
    assert len(scan) <= ref.bound_bytes(h, w, channels)
    blob = ref.jfif(scan, h, w, channels, quality)
    assert blob == harness._jpeg_header(h, w, channels == 3, quality) + scan + b'\xff\xd9'
    with Image.open(io.BytesIO(blob)) as opened:
        assert opened.size == (w, h) and opened.mode == ('RGB' if channels == 3 else 'L') and opened.format == 'JPEG'
        pixels = numpy.asarray(opened)
    assert pixels.shape == image.shape
    parsed = ref.parse(blob)
    mcu, per_row, rows, blocks = ref.geometry(h, w, channels)
    assert parsed['restart_interval'] == per_row and parsed['restart_markers'] == [r % 8 for r in range(rows - 1)]
    coded = ref.levels(image, quality)
    if channels == 1:
        assert numpy.array_equal(parsed['levels'][0], coded)
    else:
        coded = coded.reshape(rows, per_row, 6, 64)
        for i in range(4):
            assert numpy.array_equal(parsed['levels'][0][i >> 1::2, i & 1::2], coded[:, :, i])
        assert numpy.array_equal(parsed['levels'][1], coded[:, :, 4]) and numpy.array_equal(parsed['levels'][2], coded[:, :, 5])
    # the project's decoder and PIL's agree on what the file says (PIL interpolates chroma: compared on grey only)
    own = ref.decode(blob)
    assert own.shape == image.shape
    if channels == 1:
        assert numpy.abs(own.astype(int) - pixels.astype(int)).max() <= 1


def test_the_cases_have_the_properties_they_are_there_for():
    assert b'\xff\x00' in ref.expected('16x1008 colour noise')[2]
    for name in ('checkerboard grey', 'checkerboard colour'):
        symbols = ref.expected(name)[3]
        assert max(size for kind, size in symbols if kind == 'dc') == 11 and max(s & 15 for kind, s in symbols if kind == 'ac') == 10
    symbols = ref.expected('basis patterns')[3]
    assert symbols[:6] == [('dc', 0), ('ac', 0xF0), ('ac', 0xF0), ('ac', 0xF0), ('ac', 14 << 4 | 3), ('dc', 0)]          # three ZRL, no EOB
    image, quality = ref.expected('basis patterns')[:2]
    first = ref.levels(image, quality)[0, 0]
    assert first[63] != 0 and not first[:63].any()
    assert ref.geometry(147, 40, 3)[2] == 10 and ref.geometry(16, 1008, 3)[3] == 378


FIXTURES = {'smooth': lambda: png_reference.smooth(96, 128), 'textured': lambda: ref.textured(96, 128), 'noise': lambda: ref.noise(96, 128),
            'smooth grey': lambda: png_reference.smooth(96, 128, 1), 'textured grey': lambda: ref.textured(96, 128, 1),
            'noise grey': lambda: ref.noise(96, 128, 1)}


@pytest.mark.parametrize('quality', [50, 90])
@pytest.mark.parametrize('name', list(FIXTURES))
def test_quality_and_size_are_pils_at_the_same_setting(name, quality):
    from PIL import Image

    def pil_decode(blob):
        with Image.open(io.BytesIO(blob)) as opened:
            return numpy.asarray(opened)

    image = FIXTURES[name]()
    h, w = image.shape[:2]
    channels = 3 if image.ndim == 3 else 1
    ours = ref.encode(image, quality)
    blob = io.BytesIO()
    Image.fromarray(image).save(blob, 'JPEG', quality=quality, subsampling=2, optimize=False)
    theirs = blob.getvalue()
    ours_db, theirs_db = ref.psnr(pil_decode(ours), image), ref.psnr(pil_decode(theirs), image)
    rows = ref.geometry(h, w, channels)[2]
    structure = 6 + rows * (3 + (8 if channels == 3 else 3)) - 2
    excess = (len(ours) - structure - len(theirs)) / len(theirs)
    print(f'{name}, quality {quality}: PSNR ours {ours_db:.4f} dB, PIL {theirs_db:.4f} dB; {len(ours)} bytes, PIL {len(theirs)}, '
          f'structure {structure}, excess {excess:+.4f}')
    assert theirs_db - ours_db <= PSNR_SHORTFALL_DB
    assert excess <= SIZE_EXCESS
    if channels == 1:
        mine, pil = ref.parse(ours), ref.parse(theirs)
        assert numpy.array_equal(mine['quant'][0], pil['quant'][0])
        exact = ref.exact_levels(ref.planes(image)[0], mine['quant'][0])
        share_ours, share_pil = float(numpy.mean(mine['levels'][0] != exact)), float(numpy.mean(pil['levels'][0] != exact))
        print(f'    levels that differ from round(float64 DCT / q): ours {share_ours:.5f}, PIL {share_pil:.5f}')
        assert numpy.abs(mine['levels'][0] - exact).max() <= 1
        assert share_ours - share_pil <= LEVEL_SHARE_EXCESS


# ------------------------------------------------------------------------------------------------ the container
def test_avi_container_of_four_frames():
    frames = [ref.encode(ref.textured(33, 17, seed=s), 90) for s in (0, 4, 5, 6)]
    assert any(len(f) & 1 for f in frames) and any(not len(f) & 1 for f in frames)          # both parities of the padding
    blob = harness._avi_bytes(frames, 33, 17, 15)
    walked = ref.walk_avi(blob)
    micro, _, _, flags, count, _, streams, largest, width, height = walked['avih'][:10]
    assert (micro, count, streams, width, height) == (66667, 4, 1, 17, 33) and flags & 0x10 and largest == max(len(f) for f in frames)
    assert walked['strh'][6:8] == (1, 15) and walked['strh'][9] == 4          # dwScale, dwRate, dwLength
    assert walked['strf'][:5] == (40, 17, 33, 1, 24)
    assert walked['frames'] == frames
    for data in walked['frames']:
        assert data[:2] == b'\xff\xd8' and data[-2:] == b'\xff\xd9' and ref.decode(data).shape == (33, 17, 3)
    assert ref.walk_avi(harness._avi_bytes([], 33, 17, 15))['frames'] == []
    assert ref.walk_avi(harness._avi_bytes(frames[:1], 33, 17, 29.97))['strh'][6:8] == (100, 2997)
    with pytest.raises(RuntimeError, match='frame_rate'):
        harness._avi_bytes(frames, 33, 17, 0)


def test_save_video_leaves_an_existing_file_alone_and_refuses_host_arrays(tmp_path):
    path = tmp_path / 'PredictedVideo.avi'
    path.write_bytes(b'kept')
    harness.save_video(path, numpy.zeros((2, 8, 8, 3), dtype=numpy.uint8))          # (returns before it looks at the frames)
    assert path.read_bytes() == b'kept'
    image = ref.textured(8, 8)
    for call in (lambda: harness.save_video(tmp_path / 'a.avi', image[None]),
                 lambda: harness.save_video(tmp_path / 'a.avi', torch.from_numpy(image[None])),
                 lambda: harness.jpeg_files(image[None]),
                 lambda: harness.jpeg_files(torch.from_numpy(image[None]), 50)):
        with pytest.raises(RuntimeError, match='JPEG encoder takes tensors that are on the device.*no host encoder'):
            call()
    assert not (tmp_path / 'a.avi').exists()
    for binding in ops.JPEG_BINDINGS:
        with pytest.raises(RuntimeError, match='expected a tensor on the GPU'):
            ops.jpeg_scan(torch.from_numpy(image[None]), 90, binding=binding)
    with pytest.raises(RuntimeError, match="binding: expected 'ctypes' or 'torch_ext'"):
        ops.jpeg_scan(torch.from_numpy(image[None]), 90, binding='pybind')


def test_video_frame_nums_select_and_order_frames_as_numpy_does():
    """``video_frames[video_frame_nums]`` (src/NerfLlffTrainerTester01.py:166-167)."""
    frames = numpy.arange(5 * 2 * 3 * 3, dtype=numpy.uint8).reshape(5, 2, 3, 3)
    tensor = torch.from_numpy(frames)
    assert harness._select_video_frames(tensor, None) is tensor
    for nums in ([4, 0, 2], [1, 1, 3, 0, 0], numpy.array([3.0, 2.0]), numpy.loadtxt(io.StringIO('2,0,4,4'), delimiter=',').astype(int),
                 [-1, 0], [], numpy.array([[1, 2], [3, 4]])):
        expected = frames[numpy.asarray(nums).astype(int).reshape(-1)]
        assert numpy.array_equal(harness._select_video_frames(tensor, nums).numpy(), expected)
    with pytest.raises(IndexError):
        harness._select_video_frames(tensor, [5])
    with pytest.raises(IndexError):
        harness._select_video_frames(tensor, [-6])
