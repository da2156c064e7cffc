"""The PNG encoder's workgroup programs on the host: tests/native/png_coder_host.cpp runs the text of csrc/png_coder.h that the
kernels run (a phase is a loop over the 256 threads) with the buffers, sizes and offsets of snerf_png_deflate, built with the
address and undefined-behaviour sanitizers where the compiler has them, on the inputs of tests/test_gpu_png.py.  No GPU: what this
cannot see is what depends on threads running at once (a barrier that is missing, a race inside a phase)."""
import os
import shutil
import struct
import subprocess

import numpy
import pytest

from tests import png_reference as ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, 'tests', 'native', 'png_coder_host.cpp')


@pytest.fixture(scope='module')
def program(tmp_path_factory):
    compiler = shutil.which('g++') or shutil.which('c++') or shutil.which('clang++')
    assert compiler, 'no host C++ compiler'
    exe = str(tmp_path_factory.mktemp('png_coder') / 'png_coder_host')
    base = [compiler, '-std=c++17', '-O1', '-g', SRC, '-o', exe]
    r = subprocess.run(base + ['-fsanitize=address,undefined', '-fno-sanitize-recover=undefined'], capture_output=True, text=True)
    if r.returncode != 0:          # (a compiler without the sanitizer runtimes)
        r = subprocess.run(base, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def encode(program, directory, images, mode):
    images = numpy.ascontiguousarray(images)
    count, h, w = images.shape[:3]
    channels = 3 if images.ndim == 4 else 1
    images.tofile(directory / 'pixels')
    r = subprocess.run([program, str(directory / 'pixels'), str(count), str(h), str(w), str(channels), str(mode), str(directory / 'streams')],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    blob, pos, streams = (directory / 'streams').read_bytes(), 0, []
    for _ in range(count):
        n, = struct.unpack('<Q', blob[pos:pos + 8])
        streams.append(blob[pos + 8:pos + 8 + n])
        pos += 8 + n
    assert pos == len(blob)
    return streams


CASES = {
    'one grey pixel': (lambda: numpy.array([[[7]]], dtype=numpy.uint8), -1),
    'one rgb pixel': (lambda: numpy.array([[[[7, 8, 9]]]], dtype=numpy.uint8), -1),
    'noise': (lambda: ref.noise(37, 53)[None], -1),
    'smooth, two strips': (lambda: ref.smooth(96, 128)[None], -1),
    'white': (lambda: numpy.full((1, 64, 300), 255, dtype=numpy.uint8), -1),
    'white, unfiltered': (lambda: numpy.full((1, 64, 300), 255, dtype=numpy.uint8), 0),
    'run lengths': (lambda: ref.runs_row()[None], 0),
    'fibonacci counts': (lambda: ref.fibonacci_row()[None], 0),
    'fibonacci chain': (lambda: ref.fibonacci_row(chain=True)[None], 0),
    'eight frames': (lambda: numpy.stack([ref.smooth(24, 32, seed=s) for s in range(8)]), -1),
    'paeth, grey': (lambda: ref.smooth(16, 20, 1, seed=5)[None], 4),
    'average, rgb': (lambda: ref.smooth(16, 20, seed=5)[None], 3),
}


@pytest.mark.parametrize('name', list(CASES))
def test_host_run_of_the_coder_decodes(program, tmp_path, name):
    make, mode = CASES[name]
    images = make()
    for image, stream in zip(images, encode(program, tmp_path, images, mode)):
        h, w = image.shape[:2]
        channels = 3 if image.ndim == 3 else 1
        assert len(stream) <= ref.bound_bytes(h, w, channels)
        pixels, kinds = ref.decode(ref.container(stream, h, w, channels))
        assert numpy.array_equal(pixels, image)
        assert kinds == ([mode] * h if mode >= 0 else ref.adaptive_kinds(image))
        strips = ref.check_contract(stream, ref.raw_bytes(h, w, channels))
        if name == 'run lengths':
            assert tuple(length for _, length, _ in strips[0]['matches']) == ref.RUN_MATCHES
        if name.startswith('fibonacci'):
            counts = numpy.bincount(numpy.concatenate([[0], image[0], [256]]))          # filter byte, pixels, end of block
            assert ref.huffman_depth(counts) == (20 if name == 'fibonacci chain' else 11)
            assert strips[0]['type'] == 2 and max(strips[0]['lengths']) <= 15 and not strips[0]['matches']
        if name == 'noise':
            assert [b['type'] for b in strips] == [0]
