"""What the validation tests share: the fixtures of tools/make_golden_validation.py rebuilt in the loader's layout, the numpy
expressions of the reference's two 8-bit conversions (src/Trainer01.py:384-387, :397-409) and the inverse of the harness's PNG
writer."""
import json
import struct
import zlib

import numpy

from tests import util

CASES = ('ndc', 'world')
COLUMNS = ('x', 'y', 'depth', 'reprojection_error')
BATCH_KEYS_OF_THIS_BUILD = {'global_rows'}        # BatchAssembler's documented addition to the reference's batch


def load_prep(name: str):
    """-> (fixture arrays, configs, the training views' raw_data_dict, the held-out views' raw_data_dict)."""
    g = util.load(f'validation_prep_{name}.npz')
    configs = json.loads(str(g['configs_json']))
    raws = []
    for tag in ('train', 'val'):
        raw = {'frame_nums': g[f'raw_{tag}_frame_nums'].copy(),
               'nerf_data': {k: g[f'raw_{tag}_{k}'].copy() for k in ('images', 'extrinsics', 'intrinsics', 'bounds')}}
        raw['nerf_data']['resolution'] = tuple(int(x) for x in g[f'raw_{tag}_resolution'])
        frames = sorted({int(k.split('_')[3]) for k in g if k.startswith(f'raw_{tag}_sparse_')})
        if frames:
            raw['sparse_depth_data'] = {f: {c: g[f'raw_{tag}_sparse_{f}_{c}'].copy() for c in COLUMNS} for f in frames}
        if f'raw_{tag}_dense_depth_values' in g:
            raw['dense_depth_data'] = {k: g[f'raw_{tag}_dense_{k}'].copy() for k in ('depth_values', 'depth_weights')}
        raws.append(raw)
    return g, configs, raws[0], raws[1]


def model_configs(g) -> dict:
    return json.loads(str(g['model_configs_json']))


def written(g, tag: str) -> dict:
    """{file name relative to the save directory: array} of what the reference wrote for preprocessor ``tag`` ('val' / 'train')."""
    return {k[len(tag) + 1:]: v for k, v in g.items() if k.startswith(tag + '/')}


def preview_u8(array) -> numpy.ndarray:
    """save_numpy_array's preview (:399), in the array's own float32 arithmetic."""
    array = numpy.asarray(array)
    assert array.dtype == numpy.float32
    return numpy.round(array / array.max() * 255).astype('uint8')


def colour_u8(array) -> numpy.ndarray:
    """save_image's conversion (:387)."""
    array = numpy.asarray(array)
    assert array.dtype == numpy.float32
    return numpy.round(array * 255).astype('uint8')


def decode_png(data: bytes) -> numpy.ndarray:
    """The inverse of harness._png_bytes: 8-bit grey or RGB, one IDAT, filter type 0 on every row."""
    assert data[:8] == b'\x89PNG\r\n\x1a\n'
    chunks, at = [], 8
    while at < len(data):
        length, tag = struct.unpack('>I4s', data[at:at + 8])
        body = data[at + 8:at + 8 + length]
        assert struct.unpack('>I', data[at + 8 + length:at + 12 + length])[0] == zlib.crc32(tag + body) & 0xFFFFFFFF
        chunks.append((tag, body))
        at += 12 + length
    assert [tag for tag, _ in chunks] == [b'IHDR', b'IDAT', b'IEND']
    w, h, depth, colour, compression, filtering, interlace = struct.unpack('>IIBBBBB', chunks[0][1])
    assert (depth, compression, filtering, interlace) == (8, 0, 0, 0) and colour in (0, 2)
    channels = 3 if colour == 2 else 1
    rows = numpy.frombuffer(zlib.decompress(chunks[1][1]), dtype=numpy.uint8).reshape(h, 1 + w * channels)
    assert (rows[:, 0] == 0).all()
    return rows[:, 1:].reshape((h, w, 3) if channels == 3 else (h, w)).copy()


def pass_weights(configs: dict, g: dict) -> dict:
    """The state dict of the validation_pass fixture's model (synth weights of its seed, the stored density heads, fine = coarse)."""
    return util.golden_params(configs, g)
