"""The field's gradient on the CPU: the tenth header group of the binding, the restated normals (tests/field_gradient_reference.py)
against central differences of the restated NDC map and on the analytic ball, the oracle's cases and the conditions the GPU tests
compare under, the PLY with normals, the native program, and the Python refusals that need no device."""
import ctypes
import os
import shutil
import subprocess

import numpy
import pytest
import torch

from simplenerf_amd import _lib, build, geometry, ops

from . import field_gradient_reference as gref
from . import field_reference as ref
from .test_field_host import test_field_header_is_the_bindings_ninth_group as field_group_is_unchanged

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------------------------ ABI and binding
def test_gradient_header_is_the_bindings_tenth_group():
    assert [os.path.relpath(path, REPO) for path in _lib.GRADIENT_HEADERS] == [os.path.join('simplenerf_amd', 'csrc', 'simplenerf_gradient.h')]
    assert set(_lib.GRADIENT_SIGNATURES) == {'snerf_mlp_input_gradient_workspace_floats', 'snerf_mlp_input_gradient', 'snerf_field_normals'}
    earlier = set(_lib.SIGNATURES) | set(_lib.ADDED_SIGNATURES) | set(_lib.SWEEP_SIGNATURES) | set(_lib.SWEEP16_SIGNATURES) \
        | set(_lib.PNG_SIGNATURES) | set(_lib.JPEG_SIGNATURES) | set(_lib.FUSE_SIGNATURES) | set(_lib.MESH_SIGNATURES) | set(_lib.FIELD_SIGNATURES)
    assert not earlier & set(_lib.GRADIENT_SIGNATURES)
    desc = ctypes.POINTER(_lib.MlpDesc)
    assert _lib.GRADIENT_SIGNATURES['snerf_mlp_input_gradient_workspace_floats'] == (ctypes.c_size_t, [desc, ctypes.c_longlong])
    restype, argtypes = _lib.GRADIENT_SIGNATURES['snerf_mlp_input_gradient']
    assert restype == ctypes.c_int and len(argtypes) == 11 and argtypes[0] == desc and argtypes[1] == ctypes.c_void_p
    assert argtypes[2] == ctypes.POINTER(ctypes.c_void_p) and argtypes[3] == ctypes.c_int and argtypes[7] == ctypes.c_longlong
    assert argtypes[4:7] == [ctypes.c_void_p] * 3 and argtypes[8:] == [ctypes.c_void_p] * 3
    assert _lib.GRADIENT_SIGNATURES['snerf_field_normals'] == (
        ctypes.c_int, [ctypes.c_void_p] * 2 + [ctypes.c_longlong, ctypes.c_int] + [ctypes.c_double] * 3 + [ctypes.c_void_p] * 2)
    assert _lib.ABI_VERSION == 10
    field_group_is_unchanged()


@pytest.mark.skipif(shutil.which(build.HIPCC) is None and not os.path.exists(build.HIPCC), reason='hipcc not available')
def test_gradient_symbols_are_exported():
    build.build_library()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in _lib.GRADIENT_SIGNATURES:
        assert hasattr(lib, name), name


@pytest.mark.skipif(shutil.which(build.HIPCC) is None and not os.path.exists(build.HIPCC), reason='hipcc not available')
def test_workspace_query_names_what_it_refuses():
    """The size query needs no device: 0 and a message for a layered shape and a predict_visibility MLP, a size that grows by the
    dY tiles of a 128-sample workgroup and three zeros a point for the fused shapes."""
    from simplenerf_amd import synth
    build.build_library()
    lib = _lib.load()
    size = lib.snerf_mlp_input_gradient_workspace_floats
    fused = ops.mlp_desc(synth.mlp_config(64))
    one, more = size(ctypes.byref(fused), 1), size(ctypes.byref(fused), 129)
    rows = 9 * 256 + 128 + 32                                              # MlpPlan::grad_rows of the 8 x 256 / 128 MLP
    assert one > 0 and more - one == 4 * rows * 32 + 3 * 128
    assert size(ctypes.byref(fused), 0) == 0 and size(ctypes.byref(fused), -5) == 0
    for cfg, word in ((synth.mlp_config(64, depth=6, width=96, views_width=48, views_depth=3), 'layered'),
                      (synth.mlp_config(64, predict_visibility=True), 'predict_visibility')):
        assert size(ctypes.byref(ops.mlp_desc(cfg)), 100) == 0
        assert word in lib.snerf_last_error().decode(), lib.snerf_last_error()


# ------------------------------------------------------------------------------------------------------------------ the normals
def test_normals_without_ndc_are_the_negated_unit_gradient():
    rng = numpy.random.default_rng(1)
    points = rng.uniform(-2, 2, (50, 3)).astype(numpy.float32)
    grad = rng.standard_normal((50, 3)).astype(numpy.float32)
    grad[7] = 0.0
    grad[8] = [numpy.inf, 1.0, 0.0]
    grad[9] = [numpy.nan, 1.0, 0.0]
    got = gref.normals(points, grad)
    with numpy.errstate(invalid='ignore'):
        want = -grad.astype(numpy.float64) / numpy.linalg.norm(grad.astype(numpy.float64), axis=1, keepdims=True)
    keep = numpy.ones(50, dtype=bool)
    keep[7:10] = False
    assert numpy.abs(got[keep] - want[keep]).max() <= 1e-7 and not got[7:10].any()
    assert numpy.abs(numpy.linalg.norm(got[keep].astype(numpy.float64), axis=1) - 1.0).max() <= 2e-7


def test_ndc_pull_back_against_central_differences():
    """G = J^T g of the restated rule against central differences of the restated map Q(P): for a linear field s(Q) = g . Q the
    gradient of s(Q(P)) with respect to P is J^T g, and its central difference has a step error of h^2 |Q'''| / 6."""
    _, _, ndc = ref.fern_cameras()
    near = ndc[2]
    rng = numpy.random.default_rng(2)
    worst = 0.0
    for _ in range(200):
        P = [float(rng.uniform(-1.5, 1.5)), float(rng.uniform(-1.5, 1.5)), float(-near - rng.uniform(0.05, 6.0))]
        g = [float(v) for v in rng.standard_normal(3)]
        G = gref.pull_back(P, g, ndc)
        h = 1e-5 * max(1.0, abs(P[2]))
        for a in range(3):
            lo, hi = list(P), list(P)
            lo[a] -= h
            hi[a] += h
            s_lo = sum(x * y for x, y in zip(g, gref.ndc_map(lo, ndc)))
            s_hi = sum(x * y for x, y in zip(g, gref.ndc_map(hi, ndc)))
            scale = max(abs(v) for v in G) + 1e-12
            worst = max(worst, abs((s_hi - s_lo) / (2 * h) - G[a]) / scale)
    print(f'ndc pull-back against central differences: worst relative difference {worst:.3e}')
    # the step's truncation h^2 / P_z^2 ~ 1e-10 and the differences' rounding 1e-16 / h ~ 1e-11 .. 1e-10, both relative
    assert worst <= 1e-7, worst
    # the normal is minus that, normalised; behind the near plane and for a NaN depth there is none
    P = numpy.array([[0.3, -0.2, -near - 1.0], [0.3, -0.2, -near + 1e-3], [0.3, -0.2, numpy.nan]], dtype=numpy.float32)
    g = numpy.array([[1.0, 2.0, -3.0]] * 3, dtype=numpy.float32)
    got = gref.normals(P, g, ndc)
    G = numpy.array(gref.pull_back([float(v) for v in P[0]], [1.0, 2.0, -3.0], ndc))
    assert numpy.abs(got[0] + G / numpy.linalg.norm(G)).max() <= 1e-7 and not got[1:].any()


def test_the_analytic_balls_normals_point_outwards():
    rng = numpy.random.default_rng(3)
    directions = rng.standard_normal((200, 3))
    directions /= numpy.linalg.norm(directions, axis=1, keepdims=True)
    points = (directions * rng.uniform(0.1, 1.1, (200, 1))).astype(numpy.float32)
    got = gref.normals(points, gref.ball_gradient(points))
    radial = points.astype(numpy.float64) / numpy.linalg.norm(points.astype(numpy.float64), axis=1, keepdims=True)
    assert numpy.abs(got - radial).max() <= 2e-7
    outside = (directions * 1.5).astype(numpy.float32)
    assert not gref.normals(outside, gref.ball_gradient(outside)).any()          # sigma = 0 there: no gradient, no normal


# ------------------------------------------------------------------------------------------------------------------ the oracle's cases
@pytest.mark.parametrize('name', sorted(gref.CASES))
def test_oracle_cases_meet_the_comparison_conditions(name):
    case = gref.case(name)
    left_out, positive, measured = gref.RECORDED[name]
    print(f'{name}: left out {case["left_out"]:.3f}, sigma > 0 on {case["positive"]:.3f} of the compared, float32 oracle error '
          f'{case["measured"]:.3e} of max |grad| = {case["scale"]:.3e}, bound {case["bound"]:.3e}')
    assert case['left_out'] <= 0.25 and case['positive'] >= 0.5
    assert abs(case['left_out'] - left_out) <= 0.005 and abs(case['positive'] - positive) <= 0.005
    assert case['compared'][0] and case['sigma'][0] > 0                        # the one-point call is compared, and has a gradient
    assert 0.25 * measured <= case['measured'] <= 4 * measured                 # (the float32 sums' order differs between hosts)
    assert numpy.isfinite(case['grad']).all() and not case['grad'][case['sigma'] == 0].any()
    if name != 'w256_ptsaug':
        assert (case['sigma'][:129] == 0).any()                                # closed densities inside the first workgroups


# ------------------------------------------------------------------------------------------------------------------ the PLY
def parse_ply_mesh_with_normals(data):
    header, body = data.split(b'end_header\n', 1)
    lines = header.decode('ascii').split('\n')
    assert lines[:2] == ['ply', 'format binary_little_endian 1.0']
    assert lines[3:12] == [f'property float {a}' for a in ('x', 'y', 'z', 'nx', 'ny', 'nz')] + [f'property uchar {c}' for c in ('red', 'green', 'blue')]
    assert lines[-2] == 'property list uchar int vertex_indices' and len(lines) == 15
    nv, nf = int(lines[2].split()[-1]), int(lines[-3].split()[-1])
    assert lines[2] == f'element vertex {nv}' and lines[-3] == f'element face {nf}' and len(body) == nv * 27 + nf * 13
    return numpy.frombuffer(body[:nv * 27], dtype=geometry.PLY_VERTEX_NORMAL), numpy.frombuffer(body[nv * 27:], dtype=geometry.PLY_FACE)


def todays_ply_mesh_bytes(points, colours, triangles):
    """The file before normals existed, written out again from the format's own words."""
    header = ('ply\nformat binary_little_endian 1.0\n' + f'element vertex {len(points)}\nproperty float x\nproperty float y\nproperty float z\n'
              + 'property uchar red\nproperty uchar green\nproperty uchar blue\n'
              + f'element face {len(triangles)}\nproperty list uchar int vertex_indices\nend_header\n').encode('ascii')
    body = b''.join(numpy.asarray(p, '<f4').tobytes() + numpy.asarray(c, 'u1').tobytes() for p, c in zip(points, colours))
    body += b''.join(b'\x03' + numpy.asarray(t, '<i4').tobytes() for t in triangles)
    return header + body


def test_ply_with_normals_parses_back_and_without_is_unchanged(tmp_path):
    rng = numpy.random.default_rng(4)
    points = rng.standard_normal((7, 3)).astype(numpy.float32)
    normals = rng.standard_normal((7, 3)).astype(numpy.float32)
    colours = rng.integers(0, 256, (7, 3)).astype(numpy.uint8)
    triangles = rng.integers(0, 7, (5, 3)).astype(numpy.int32)
    plain = geometry.ply_mesh_bytes(points, colours, triangles)
    assert plain == todays_ply_mesh_bytes(points, colours, triangles) == geometry.ply_mesh_bytes(points, colours, triangles, None)
    data = geometry.ply_mesh_bytes(torch.from_numpy(points), colours, torch.from_numpy(triangles), torch.from_numpy(normals))
    assert len(data) - len(plain) == 7 * 12 + len(b'property float nx\nproperty float ny\nproperty float nz\n')
    records, faces = parse_ply_mesh_with_normals(data)
    assert numpy.array_equal(numpy.stack([records[k] for k in ('x', 'y', 'z')], axis=1), points)
    assert numpy.array_equal(numpy.stack([records[k] for k in ('nx', 'ny', 'nz')], axis=1), normals)
    assert numpy.array_equal(numpy.stack([records[k] for k in ('red', 'green', 'blue')], axis=1), colours)
    assert numpy.array_equal(numpy.stack([faces[k] for k in ('a', 'b', 'c')], axis=1), triangles) and (faces['count'] == 3).all()
    empty = geometry.ply_mesh_bytes(points[:0], colours[:0], triangles[:0], normals[:0])
    assert parse_ply_mesh_with_normals(empty)[0].shape == (0,)
    geometry.save_ply_mesh(tmp_path / 'a.ply', points, colours, triangles, normals)
    geometry.save_ply_mesh(tmp_path / 'b.ply', points, colours, triangles)
    assert (tmp_path / 'a.ply').read_bytes() == data and (tmp_path / 'b.ply').read_bytes() == plain
    for bad in (normals[:6], normals.astype(numpy.float64), normals[:, :2]):
        with pytest.raises(RuntimeError, match='normals'):
            geometry.ply_mesh_bytes(points, colours, triangles, bad)


# ------------------------------------------------------------------------------------------------------------------ the native program
@pytest.mark.skipif(shutil.which(build.HIPCC) is None and not os.path.exists(build.HIPCC), reason='hipcc not available')
def test_gradient_abi_program_compiles_and_links(tmp_path):
    """CPU-side half of the native smoke: the new header is valid C++ for an outside consumer and the three symbols link."""
    build.build_library()
    assert os.path.exists(compile_smoke(str(tmp_path)))


def compile_smoke(out_dir):
    exe = os.path.join(out_dir, 'gradient_abi_smoke')
    lib_dir = os.path.dirname(_lib.LIB_PATH)
    cmd = [build.HIPCC, '--offload-arch=gfx950', '-O1', '-std=c++17', f'-I{os.path.join(REPO, "include")}', f'-I{build.CSRC}',
           os.path.join(REPO, 'tests', 'native', 'gradient_abi_smoke.cpp'), '-o', exe, f'-L{lib_dir}', '-lsimplenerf_hip',
           f'-Wl,-rpath,{lib_dir}']
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def native_fixture(count=300) -> bytes:
    """What tests/native/gradient_abi_smoke.cpp reads, little-endian: int32 count, params | float64 cx, cy, near | float32 points
    (count, 3) | float32 the float64 oracle's gradient (count, 3) | uint8 compared (count) | float32 tolerance (absolute, on the
    gradient) | per parameter: int64 its number of floats, float32 its values -- the seeded 8 x 128 / 64 case of
    tests/field_gradient_reference.py."""
    import struct

    from simplenerf_amd import synth
    case = gref.case('w128_views')
    _, _, ndc = ref.fern_cameras()
    params = [p.numpy() for p in synth.abi_param_list(gref.case_state('w128_views'), gref.PREFIX)]
    little = lambda array, dtype: numpy.ascontiguousarray(array).astype(dtype).tobytes()
    parts = [struct.pack('<2i3d', count, len(params), *ndc), little(case['points'][:count], '<f4'), little(case['grad'][:count], '<f4'),
             little(case['compared'][:count], 'u1'), struct.pack('<f', case['bound'] * case['scale'])]
    for value in params:
        parts += [struct.pack('<q', value.size), little(value, '<f4')]
    return b''.join(parts)


def test_native_fixture_layout():
    data = native_fixture(33)
    assert numpy.frombuffer(data[:8], '<i4').tolist() == [33, 24]
    assert len(data) == 8 + 24 + 33 * 25 + 4 + sum(8 + 4 * v.numel() for k, v in gref.case_state('w128_views').items())


# ------------------------------------------------------------------------------------------------------------------ refusals
def test_python_refusals_without_a_device():
    with pytest.raises(RuntimeError, match='GPU'):
        ops.field_normals(torch.zeros((4, 3)), torch.zeros((4, 3)))
    with pytest.raises(RuntimeError, match='GPU'):
        geometry.field_normals(lambda p: p, torch.zeros((4, 3)))
    from simplenerf_amd.models.ModelFactory import get_model
    model = get_model(gref.case_configs('w128_views'), None)
    with pytest.raises(RuntimeError, match='GPU'):
        model.query_gradient(torch.zeros((4, 3)))
    with pytest.raises(RuntimeError, match='point_block'):
        model.query_gradient(torch.zeros((4, 3)), point_block=0)
    with pytest.raises(KeyError, match='mlp'):
        model.query_gradient(torch.zeros((4, 3)), mlp='fine_mlp')
