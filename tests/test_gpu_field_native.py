"""The density mesh from the C ABI alone: tests/native/field_abi_smoke.cpp is compiled against include/simplenerf_hip.h and
simplenerf_amd/csrc/simplenerf_field.h, linked with libsimplenerf_hip.so and run on the GPU without PyTorch in the process; it reads
the analytic scene's cameras, the restated points and weights of a grid over it and a seeded MLP from the fixture written here
(field_reference.native_fixture), and must print the counts the restatement gives for the volume of the same densities.
(tests/test_field_host.py compiles and links the program without a GPU.)"""
import subprocess

import numpy
import pytest
import torch

from simplenerf_amd import ops

from . import field_reference as ref
from . import mesh_reference
from .test_field_host import compile_smoke

DEV = 'cuda:0'


@pytest.mark.gpu
def test_field_abi_program_gives_the_restatements_counts(tmp_path):
    exe = compile_smoke(str(tmp_path))
    # the densities the program will see: the same fp32 forward on the same points, through the Python binding
    cfg, params = ref.native_mlp()
    mlp = ops.PackedMlp(cfg, DEV)
    mlp.pack([torch.from_numpy(p).to(DEV) for p in params], ops.PRECISION_FP32, False)
    want_points, want_weight, _ = ref.scene_grid_points()
    points = torch.from_numpy(numpy.array(want_points)).to(DEV)
    down = torch.tensor([0.0, 0.0, -1.0], device=DEV).expand(len(points), 3).contiguous()
    sigma = mlp.forward(points, torch.zeros_like(points), down, torch.zeros((len(points), 1), device=DEV))[0].reshape(-1).cpu().numpy()
    level = float(numpy.median(sigma[sigma > 0]))
    nx, ny, nz = ref.SMALL_EXTENTS
    tsdf = ref.values(sigma.reshape(nz, ny, nx), want_weight.reshape(nz, ny, nx), level)
    vertices, triangles, _, _ = mesh_reference.extract_mesh(tsdf, want_weight.reshape(nz, ny, nx), ref.SMALL_LO, ref.SMALL_VOXEL)
    assert len(vertices) > 0 and len(triangles) > 0
    (tmp_path / 'fixture').write_bytes(ref.native_fixture(level, (len(vertices), len(triangles))))
    r = subprocess.run([exe, str(tmp_path / 'fixture')], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0 and 'field_abi_smoke: OK' in r.stdout, r.stdout + r.stderr
    assert f'field_abi_smoke: 1716 nodes, {int((want_weight > 0).sum())} seen' in r.stdout
    assert f'field_abi_smoke: 1716 nodes, {len(vertices)} vertices, {len(triangles)} triangles' in r.stdout
