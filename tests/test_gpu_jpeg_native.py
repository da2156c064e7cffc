"""The JPEG encoder from the C ABI alone: tests/native/jpeg_abi_smoke.cpp is compiled against include/simplenerf_hip.h and
simplenerf_amd/csrc/simplenerf_jpeg.h, linked with libsimplenerf_hip.so and run on the GPU without PyTorch in the process; it
compares the scan of one frame with the bytes passed in here, which are the restated encoder's (jpeg_reference)."""
import os
import shutil
import subprocess

import pytest

from simplenerf_amd import _lib, build

from . import jpeg_reference as ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, 'tests', 'native', 'jpeg_abi_smoke.cpp')


def compile_smoke(out_dir):
    exe = os.path.join(out_dir, 'jpeg_abi_smoke')
    lib_dir = os.path.dirname(_lib.LIB_PATH)
    cmd = [build.HIPCC, '--offload-arch=gfx950', '-O1', '-std=c++17', f'-I{os.path.join(REPO, "include")}', f'-I{build.CSRC}', SRC,
           '-o', exe, f'-L{lib_dir}', '-lsimplenerf_hip', f'-Wl,-rpath,{lib_dir}']
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


@pytest.mark.skipif(shutil.which(build.HIPCC) is None and not os.path.exists(build.HIPCC), reason='hipcc not available')
def test_jpeg_abi_program_compiles_and_links(tmp_path):
    """CPU-side half: the new header is valid C++ for an outside consumer and the three symbols link."""
    build.build_library()
    assert os.path.exists(compile_smoke(str(tmp_path)))


@pytest.mark.gpu
def test_jpeg_abi_program_gives_the_restated_encoders_bytes(tmp_path):
    exe = compile_smoke(str(tmp_path))
    for name in ('17x33 colour', '23x300 grey, two chunks'):
        image, quality, scan, _ = ref.expected(name)
        image.tofile(tmp_path / 'pixels')
        (tmp_path / 'expected').write_bytes(scan)
        h, w = image.shape[:2]
        r = subprocess.run([exe, str(tmp_path / 'pixels'), str(h), str(w), str(3 if image.ndim == 3 else 1), str(quality),
                            str(tmp_path / 'expected')], capture_output=True, text=True, timeout=120)
        print(r.stdout)
        assert r.returncode == 0 and 'jpeg_abi_smoke: OK' in r.stdout, name + r.stdout + r.stderr
