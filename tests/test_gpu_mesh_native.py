"""The mesh export from the C ABI alone: tests/native/mesh_abi_smoke.cpp is compiled against include/simplenerf_hip.h and
simplenerf_amd/csrc/simplenerf_mesh.h, linked with libsimplenerf_hip.so and run on the GPU without PyTorch in the process; it reads
the analytic scene and the restatement's volume, mesh and colours from the fixture written here (mesh_reference.native_fixture) and
checks the volume, both counts and the first and last record of every output.  (tests/test_mesh_host.py compiles and links the
program without a GPU.)"""
import subprocess

import pytest

from . import mesh_reference as ref
from .test_mesh_host import compile_smoke


@pytest.mark.gpu
def test_mesh_abi_program_gives_the_restatements_records(tmp_path):
    exe = compile_smoke(str(tmp_path))
    (tmp_path / 'fixture').write_bytes(ref.native_fixture())
    r = subprocess.run([exe, str(tmp_path / 'fixture')], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0 and 'mesh_abi_smoke: OK' in r.stdout, r.stdout + r.stderr
    assert 'integrated 15625 nodes, 15269 observed' in r.stdout
    assert 'counted 3736 vertices and 7468 triangles' in r.stdout and 'coloured 3736 vertices' in r.stdout
