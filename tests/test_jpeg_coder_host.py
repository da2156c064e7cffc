"""The JPEG encoder's workgroup programs on the host: tests/native/jpeg_coder_host.cpp runs the text of csrc/jpeg_coder.h that the
kernels run (a phase is a loop over the 256 threads) with the buffers, sizes and offsets of snerf_jpeg_scan, built with the address
and undefined-behaviour sanitizers where the compiler has them, on the inputs of tests/test_gpu_jpeg.py; its scans equal the
restated encoder's (tests/jpeg_reference.py) byte for byte.  No GPU: what this cannot see is what depends on threads running at
once (a barrier that is missing, a race inside a phase)."""
import os
import shutil
import struct
import subprocess

import numpy
import pytest

from tests import jpeg_reference as ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, 'tests', 'native', 'jpeg_coder_host.cpp')


@pytest.fixture(scope='module')
def program(tmp_path_factory):
    compiler = shutil.which('g++') or shutil.which('c++') or shutil.which('clang++')
    assert compiler, 'no host C++ compiler'
    exe = str(tmp_path_factory.mktemp('jpeg_coder') / 'jpeg_coder_host')
    base = [compiler, '-std=c++17', '-O1', '-g', SRC, '-o', exe]
    r = subprocess.run(base + ['-fsanitize=address,undefined', '-fno-sanitize-recover=undefined'], capture_output=True, text=True)
    if r.returncode != 0:          # (a compiler without the sanitizer runtimes)
        r = subprocess.run(base, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def encode(program, directory, images, quality):
    images = numpy.ascontiguousarray(images)
    count, h, w = images.shape[:3]
    channels = 3 if images.ndim == 4 else 1
    images.tofile(directory / 'pixels')
    r = subprocess.run([program, str(directory / 'pixels'), str(count), str(h), str(w), str(channels), str(quality), str(directory / 'scans')],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    blob, pos, scans = (directory / 'scans').read_bytes(), 0, []
    for _ in range(count):
        n, = struct.unpack('<Q', blob[pos:pos + 8])
        scans.append(blob[pos + 8:pos + 8 + n])
        pos += 8 + n
    assert pos == len(blob)
    return scans


@pytest.mark.parametrize('name', list(ref.CASES))
def test_host_run_of_the_coder_equals_the_restated_encoder(program, tmp_path, name):
    image, quality, scan, _ = ref.expected(name)
    produced, = encode(program, tmp_path, image[None], quality)
    assert len(produced) <= ref.bound_bytes(image.shape[0], image.shape[1], 3 if image.ndim == 3 else 1)
    assert produced == scan


def test_three_frames_in_one_run_are_the_frames_alone(program, tmp_path):
    images = numpy.stack([ref.textured(19, 35, seed=s) if s else ref.noise(19, 35) for s in range(3)])
    together = encode(program, tmp_path, images, 75)
    assert together == [ref.scan(image, 75) for image in images] and len(set(together)) == 3
