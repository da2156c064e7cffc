"""The 16-bit view sweep from the C ABI alone: tests/native/view_sweep16_abi_smoke.cpp is compiled against include/simplenerf_hip.h
and simplenerf_amd/csrc/simplenerf_sweep16.h, linked with libsimplenerf_hip.so and run on the GPU without PyTorch in the process --
snerf_mlp_forward_train -> snerf_composite -> snerf_view_sweep_half against snerf_mlp_forward + snerf_composite per view, in f16 and
in bf16, at a tolerance the program computes from a float and a double restatement of the formula."""
import os
import shutil
import subprocess

import pytest

from simplenerf_amd import _lib, build

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, 'tests', 'native', 'view_sweep16_abi_smoke.cpp')


def compile_smoke(out_dir):
    exe = os.path.join(out_dir, 'view_sweep16_abi_smoke')
    lib_dir = os.path.dirname(_lib.LIB_PATH)
    cmd = [build.HIPCC, '--offload-arch=gfx950', '-O1', '-std=c++17', f'-I{os.path.join(REPO, "include")}', f'-I{build.CSRC}', SRC,
           '-o', exe, f'-L{lib_dir}', '-lsimplenerf_hip', f'-Wl,-rpath,{lib_dir}']
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


@pytest.mark.skipif(shutil.which(build.HIPCC) is None and not os.path.exists(build.HIPCC), reason='hipcc not available')
def test_view_sweep16_abi_program_compiles_and_links(tmp_path):
    """CPU-side half: the new header is valid C++ for an outside consumer and the three symbols link."""
    build.build_library()
    assert os.path.exists(compile_smoke(str(tmp_path)))


@pytest.mark.gpu
def test_view_sweep16_abi_program_runs_without_torch(tmp_path):
    exe = compile_smoke(str(tmp_path))
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0 and 'view_sweep16_abi_smoke: OK' in r.stdout, r.stdout + r.stderr
