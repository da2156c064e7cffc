"""The field export on the CPU: the restatement's NDC map (tests/field_reference.py) against the oracle's NDC rays, the margins that
let the GPU tests ask for exact equality, the level-set values, the header group of the binding, the native program and its
fixture, and the Python refusals that need no device."""
import ctypes
import math
import os
import shutil
import subprocess

import numpy
import pytest
import torch

from oracle import raygen_oracle
from simplenerf_amd import _lib, build, geometry, harness, ops, synth

from . import field_reference as ref
from . import mesh_reference

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARGIN = 1e-9                       # a node or point decided closer than this to a threshold may be left out of a comparison
# The largest distance, over the rays and depths of test_ndc_map_lies_on_the_oracles_ndc_rays, between the fp64 map of the world point
# and the point o_ndc + t d_ndc of the oracle's fp32 NDC ray: 2.64e-7 measured (the oracle's own fp32 rounding of o_ndc and d_ndc,
# values up to 1.3 in magnitude).  The bound is four times that.
NDC_MEASURED, NDC_BOUND = 2.64e-7, 4 * 2.64e-7


# ------------------------------------------------------------------------------------------------------------------ the input map
def test_ndc_map_lies_on_the_oracles_ndc_rays():
    camera = synth.camera('fern', 0)
    h, w = camera['resolution']
    near = camera['near']
    rays_o, rays_d = raygen_oracle.camera_rays((h, w), camera['intrinsic'], camera['pose'])
    o_ndc, d_ndc = raygen_oracle.ndc_rays(rays_o, rays_d, (h, w), camera['intrinsic'], near)
    ndc = geometry.ndc_parameters(camera)
    assert ndc[2] == near and ndc[0] == -1.0 / (w / (2.0 * float(camera['intrinsic'][0, 0])))
    assert ndc[1] == -1.0 / (h / (2.0 * float(camera['intrinsic'][1, 1])))
    worst, checked = 0.0, 0
    for y in range(0, h, 53):
        for x in range(0, w, 47):
            o, d = rays_o[y, x].astype(numpy.float64), rays_d[y, x].astype(numpy.float64)
            start = -(near + o[2]) / d[2]                                     # where the ray meets the near plane
            for beyond in (0.0, 0.37, 2.0, 25.0):
                P = (o + (start + beyond) * d).tolist()
                if beyond == 0.0:
                    P[2] = -near                                               # (exactly on the plane: still in front)
                Q, in_front, _ = ref.input_point(P, ndc)
                assert in_front
                t = 1.0 + near / P[2]                                          # the NDC depth of P on its warped ray
                want = o_ndc[y, x].astype(numpy.float64) + t * d_ndc[y, x].astype(numpy.float64)
                worst = max(worst, float(numpy.abs(numpy.array(Q) - want).max()))
                checked += 1
    print(f'ndc map against the oracle: worst distance {worst:.3e} over {checked} points [{NDC_BOUND:.1e}]')
    assert checked > 300 and worst <= NDC_BOUND, worst
    behind = ref.input_point([0.3, -0.2, -near + 1e-6], ndc)
    assert behind[0] == [0.0, 0.0, 0.0] and behind[1] is False
    assert ref.input_point([0.3, -0.2, float('nan')], ndc)[:2] == ([0.0, 0.0, 0.0], False)
    assert ref.input_point([0.3, -0.2, 5.0], None)[:2] == ([0.3, -0.2, 5.0], True)


# ------------------------------------------------------------------------------------------------------------------ the scenes
def test_scene_grid_and_its_margins():
    """The conditions under which GPU test 1 asks for every node: no decision of the 13 x 12 x 11 grid over the sphere scene within
    1e-9 of turning over.  The restated lookup agrees with mesh_reference's on every node and view."""
    points, weight, margins = ref.scene_grid_points()
    assert points.shape == (1716, 3) and points.dtype == numpy.float32 and weight.shape == (1716,) and weight.dtype == numpy.uint8
    assert min(margins) >= MARGIN, min(margins)
    assert weight.max() == 6 and 1 <= weight.min() < 6                       # (every node of this grid is seen; views = 0 covers weight 0)
    s = mesh_reference.scene()
    valid = numpy.ones(s['depth'].shape, dtype=numpy.float32)
    nx, ny, nz = ref.SMALL_EXTENTS
    for n in range(0, 1716, 7):
        P = mesh_reference.node_position(ref.SMALL_LO, ref.SMALL_VOXEL, (n % nx, n // nx % ny, n // (nx * ny)))
        assert points[n].tolist() == numpy.array(P, dtype=numpy.float32).tolist()
        seen = [mesh_reference.look_up(P, s['extrinsics'], s['intrinsics'], valid, None, u) is not None for u in range(6)]
        assert [ref.sees(P, ref.scene_table(), u, 48, 48)[0] for u in range(6)] == seen and sum(seen) == weight[n]
    blocks = [ref.grid_points(ref.SMALL_LO, ref.SMALL_VOXEL, ref.SMALL_EXTENTS, ref.scene_table(), (48, 48), None, first, count)
              for first, count in ((0, 1000), (1000, 716))]
    assert numpy.concatenate([b[0] for b in blocks]).tobytes() == points.tobytes()
    assert numpy.concatenate([b[1] for b in blocks]).tobytes() == weight.tobytes()
    none = ref.grid_points(ref.SMALL_LO, ref.SMALL_VOXEL, ref.SMALL_EXTENTS, ref.scene_table()[:0], (48, 48))
    assert not none[1].any() and none[0].tobytes() == points.tobytes()


def test_values_follow_their_sentence():
    level = 2.5
    sigma = numpy.array([0.0, level / 2, level, 2 * level, 10 * level, numpy.inf, numpy.nan], dtype=numpy.float32)
    assert ref.values(sigma, numpy.full(7, 3, numpy.uint8), level).tolist() == [1.0, 0.5, 0.0, -1.0, -1.0, -1.0, 1.0]
    assert ref.values(sigma, numpy.zeros(7, numpy.uint8), level).tolist() == [1.0] * 7
    assert ref.values(sigma.reshape(7, 1, 1), numpy.ones((7, 1, 1), numpy.uint8), level).shape == (7, 1, 1)


def test_point_views_pick_the_nearest_view_that_sees():
    table = ref.scene_table()
    points = numpy.array([[0.9, 0.0, 0.0], [-0.9, 0.1, 0.0], [0.0, 0.0, 0.95], [50.0, 50.0, 50.0]], dtype=numpy.float32)
    mlp_points, dirs, view = ref.point_views(points, table, (48, 48))
    assert view.tolist() == [0, 1, 4, ref.NO_VIEW] and mlp_points.tobytes() == points.tobytes()
    assert numpy.allclose(numpy.linalg.norm(dirs.astype(numpy.float64), axis=1), 1.0, atol=1e-6)
    centre = numpy.array(mesh_reference.SCENE_EYES[0])
    assert numpy.allclose(dirs[0], (points[0] - centre) / numpy.linalg.norm(points[0] - centre), atol=1e-6)
    assert numpy.allclose(dirs[3], (points[3] - centre) / numpy.linalg.norm(points[3] - centre), atol=1e-6)      # view 0's direction


# ------------------------------------------------------------------------------------------------------------------ ABI and binding
def test_field_header_is_the_bindings_ninth_group():
    assert [os.path.relpath(path, REPO) for path in _lib.FIELD_HEADERS] == [os.path.join('simplenerf_amd', 'csrc', 'simplenerf_field.h')]
    assert set(_lib.FIELD_SIGNATURES) == {'snerf_field_grid_points', 'snerf_field_point_views', 'snerf_field_values'}
    earlier = set(_lib.SIGNATURES) | set(_lib.ADDED_SIGNATURES) | set(_lib.SWEEP_SIGNATURES) | set(_lib.SWEEP16_SIGNATURES) \
        | set(_lib.PNG_SIGNATURES) | set(_lib.JPEG_SIGNATURES) | set(_lib.FUSE_SIGNATURES) | set(_lib.MESH_SIGNATURES)
    assert not earlier & set(_lib.FIELD_SIGNATURES)
    ndc = [ctypes.c_int] + [ctypes.c_double] * 3
    assert _lib.FIELD_SIGNATURES['snerf_field_grid_points'] == (
        ctypes.c_int, [ctypes.c_double] * 4 + [ctypes.c_int] * 3 + [ctypes.c_longlong] * 2 + [ctypes.c_void_p] + [ctypes.c_int] * 3 + ndc
        + [ctypes.c_void_p] * 3)
    assert _lib.FIELD_SIGNATURES['snerf_field_point_views'] == (
        ctypes.c_int, [ctypes.c_void_p, ctypes.c_longlong, ctypes.c_void_p] + [ctypes.c_int] * 3 + ndc + [ctypes.c_void_p] * 4)
    assert _lib.FIELD_SIGNATURES['snerf_field_values'] == (
        ctypes.c_int, [ctypes.c_void_p] * 2 + [ctypes.c_longlong, ctypes.c_double] + [ctypes.c_void_p] * 2)
    assert _lib.C.SNERF_FIELD_NO_VIEW == 255 == ops.FIELD_NO_VIEW == ref.NO_VIEW and _lib.ABI_VERSION == 10


@pytest.mark.skipif(shutil.which(build.HIPCC) is None and not os.path.exists(build.HIPCC), reason='hipcc not available')
def test_field_symbols_are_exported():
    build.build_library()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in _lib.FIELD_SIGNATURES:
        assert hasattr(lib, name), name


def test_native_fixture_layout():
    data = ref.native_fixture(3.0, (12, 34))
    assert numpy.frombuffer(data[:28], '<i4').tolist() == [6, 48, 48, 13, 12, 11, 16]
    assert numpy.frombuffer(data[28:68], '<f8').tolist() == [0.25, -1.51, -1.49, -1.503, 3.0]
    assert numpy.frombuffer(data[68:84], '<i8').tolist() == [12, 34]
    params = ref.native_mlp()[1]
    assert [p.shape for p in params[:4]] == [(128, 63), (128,), (128, 128), (128,)] and len(params) == 16
    assert len(data) == 84 + 6 * 42 * 8 + 1716 * 13 + sum(8 + 4 * p.size for p in params)
    assert numpy.frombuffer(ref.native_fixture()[68:84], '<i8').tolist() == [-1, -1]


@pytest.mark.skipif(shutil.which(build.HIPCC) is None and not os.path.exists(build.HIPCC), reason='hipcc not available')
def test_field_abi_program_compiles_and_links(tmp_path):
    """CPU-side half of the native smoke: the new header is valid C++ for an outside consumer and the three symbols link."""
    build.build_library()
    assert os.path.exists(compile_smoke(str(tmp_path)))


def compile_smoke(out_dir):
    exe = os.path.join(out_dir, 'field_abi_smoke')
    lib_dir = os.path.dirname(_lib.LIB_PATH)
    cmd = [build.HIPCC, '--offload-arch=gfx950', '-O1', '-std=c++17', f'-I{os.path.join(REPO, "include")}', f'-I{build.CSRC}',
           os.path.join(REPO, 'tests', 'native', 'field_abi_smoke.cpp'), '-o', exe, f'-L{lib_dir}', '-lsimplenerf_hip',
           f'-Wl,-rpath,{lib_dir}']
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


# ------------------------------------------------------------------------------------------------------------------ refusals
def test_python_refusals_without_a_device():
    """Every operand is checked before the library is loaded: a CPU tensor, a wrong dtype or shape, a bad grid, level or ndc."""
    table = torch.from_numpy(numpy.array(ref.scene_table()))
    grid = (ref.SMALL_LO, ref.SMALL_VOXEL, ref.SMALL_EXTENTS)
    with pytest.raises(RuntimeError, match='GPU'):
        ops.field_grid_points(*grid, table, (48, 48))
    with pytest.raises(RuntimeError, match='voxel_size'):
        ops.field_grid_points(ref.SMALL_LO, 0.0, ref.SMALL_EXTENTS, table, (48, 48))
    with pytest.raises(RuntimeError, match=r'extents.*2\^31 - 1'):
        ops.field_grid_points(ref.SMALL_LO, 0.25, (1024, 1024, 1024), table, (48, 48))
    with pytest.raises(RuntimeError, match='GPU'):
        ops.field_point_views(torch.zeros((4, 3)), table, (48, 48))
    with pytest.raises(RuntimeError, match='GPU'):
        ops.field_values(torch.zeros((4,)), torch.zeros((4,), dtype=torch.uint8), 1.0)
    camera = synth.camera('fern', 0, resolution=(48, 64))
    cx, cy, near = geometry.ndc_parameters(camera)
    assert cx < 0 and cy < 0 and near == camera['near'] and math.isclose(cy / cx, (64 / 48) * float(camera['intrinsic'][1, 1]) / float(camera['intrinsic'][0, 0]))
    sphere = mesh_reference.scene()
    query = lambda points: points[:, 0]
    for level in (0.0, -1.0, float('nan'), float('inf')):
        with pytest.raises(RuntimeError, match='level'):
            geometry.density_volume(query, *grid, sphere['extrinsics'], sphere['intrinsics'], (48, 48), level)
    with pytest.raises(RuntimeError, match='point_block'):
        geometry.density_volume(query, *grid, sphere['extrinsics'], sphere['intrinsics'], (48, 48), 1.0, point_block=0)
    with pytest.raises(RuntimeError, match=r'extents.*2\^31 - 1'):
        geometry.density_volume(query, ref.SMALL_LO, 0.25, (1024, 1024, 1024), sphere['extrinsics'], sphere['intrinsics'], (48, 48), 1.0)
    with pytest.raises(RuntimeError, match='GPU'):
        geometry.colour_vertices(lambda p, d: p, torch.zeros((4, 3)), sphere['extrinsics'], sphere['intrinsics'], (48, 48))
    cfg = synth.make_configs('config2')
    cameras = [synth.camera('fern', i, resolution=(48, 64)) for i in range(3)]
    box = ((-1.0, -1.0, -3.0), (1.0, 1.0, -1.5))
    for level in (0.0, float('nan'), float('inf')):
        with pytest.raises(RuntimeError, match='level'):
            harness.export_density_mesh(None, cfg, cameras, 'unused.ply', 'cpu', 0.25, level, box)
    with pytest.raises(RuntimeError, match='voxel_size'):
        harness.export_density_mesh(None, cfg, cameras, 'unused.ply', 'cpu', -0.25, 1.0, box)
    with pytest.raises(RuntimeError, match='no cameras'):
        harness.export_density_mesh(None, cfg, [], 'unused.ply', 'cpu', 0.25, 1.0, box)
    with pytest.raises(RuntimeError, match=r'7 nx ny nz <= 2\^31 - 1'):
        harness.export_density_mesh(None, cfg, cameras, 'unused.ply', 'cpu', 0.25 / 1000, 1.0, box)
    with pytest.raises(RuntimeError, match='bounds'):
        harness.export_density_mesh(None, cfg, cameras, 'unused.ply', 'cpu', 0.25, 1.0, (box[1], box[0]))
    other = dict(cameras[1], intrinsic=cameras[1]['intrinsic'] * numpy.float32(1.25))
    with pytest.raises(RuntimeError, match='ndc.*focal length'):
        harness.export_density_mesh(None, cfg, [cameras[0], other], 'unused.ply', 'cpu', 0.25, 1.0, box)
    with pytest.raises(RuntimeError, match='resolution'):
        harness.export_density_mesh(None, cfg, [cameras[0], synth.camera('fern', 1, resolution=(24, 32))], 'unused.ply', 'cpu', 0.25, 1.0, box)
    visible = synth.make_configs('config2')
    visible['model']['fine_mlp'] = synth.mlp_config(128, predict_visibility=True)
    with pytest.raises(NotImplementedError, match='predict_visibility'):
        harness.export_density_mesh(None, visible, cameras, 'unused.ply', 'cpu', 0.25, 1.0, box)
    assert not os.path.exists('unused.ply')
