"""The PNG encoder from the C ABI alone: tests/native/png_abi_smoke.cpp is compiled against include/simplenerf_hip.h and
simplenerf_amd/csrc/simplenerf_png.h, linked with libsimplenerf_hip.so and run on the GPU without PyTorch in the process; it wraps
each stream in the PNG container with a CRC-32 of its own and writes the files, which are decoded here (png_reference)."""
import glob
import os
import re
import shutil
import subprocess

import numpy
import pytest

from simplenerf_amd import _lib, build

from . import png_reference as ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, 'tests', 'native', 'png_abi_smoke.cpp')


def compile_smoke(out_dir):
    exe = os.path.join(out_dir, 'png_abi_smoke')
    lib_dir = os.path.dirname(_lib.LIB_PATH)
    cmd = [build.HIPCC, '--offload-arch=gfx950', '-O1', '-std=c++17', f'-I{os.path.join(REPO, "include")}', f'-I{build.CSRC}', SRC,
           '-o', exe, f'-L{lib_dir}', '-lsimplenerf_hip', f'-Wl,-rpath,{lib_dir}']
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


@pytest.mark.skipif(shutil.which(build.HIPCC) is None and not os.path.exists(build.HIPCC), reason='hipcc not available')
def test_png_abi_program_compiles_and_links(tmp_path):
    """CPU-side half: the new header is valid C++ for an outside consumer and the three symbols link."""
    build.build_library()
    assert os.path.exists(compile_smoke(str(tmp_path)))


@pytest.mark.gpu
def test_png_abi_program_writes_files_that_decode(tmp_path):
    exe = compile_smoke(str(tmp_path))
    out = tmp_path / 'files'
    out.mkdir()
    r = subprocess.run([exe, str(out)], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0 and 'png_abi_smoke: OK' in r.stdout, r.stdout + r.stderr
    files = sorted(glob.glob(str(out / '*.png')))
    assert [os.path.basename(f).split('_')[0] for f in files] == ['flat', 'grey', 'grey', 'noise', 'ramp']
    for path in files:
        h, w, c = (int(v) for v in re.search(r'_(\d+)x(\d+)x(\d+)\.png$', path).groups())
        expected = numpy.fromfile(path[:-4] + '.raw', dtype=numpy.uint8).reshape((h, w, 3) if c == 3 else (h, w))
        pixels, kinds = ref.decode(open(path, 'rb').read())
        assert pixels.shape == expected.shape and (pixels == expected).all(), path
        assert kinds == ([2] * h if 'grey_up' in path else ref.adaptive_kinds(expected)), path
        assert os.path.getsize(path) - 57 <= ref.bound_bytes(h, w, c), path          # (57 bytes of container)
