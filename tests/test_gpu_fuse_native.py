"""The point-cloud export from the C ABI alone: tests/native/fuse_abi_smoke.cpp is compiled against include/simplenerf_hip.h and
simplenerf_amd/csrc/simplenerf_fuse.h, linked with libsimplenerf_hip.so and run on the GPU without PyTorch in the process; it reads
the analytic scene and the restatement's records from the fixture written here (fuse_reference.native_fixture) and checks N, M and
the first and last record of both calls.  (tests/test_fuse_host.py compiles and links the program without a GPU.)"""
import subprocess

import pytest

from . import fuse_reference as ref
from .test_fuse_host import compile_smoke


@pytest.mark.gpu
def test_fuse_abi_program_gives_the_restatements_records(tmp_path):
    exe = compile_smoke(str(tmp_path))
    (tmp_path / 'fixture').write_bytes(ref.native_fixture())
    r = subprocess.run([exe, str(tmp_path / 'fixture')], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0 and 'fuse_abi_smoke: OK' in r.stdout, r.stdout + r.stderr
    assert 'fused 577 points of 663 pixels' in r.stdout and 'thinned to 147 voxels' in r.stdout
