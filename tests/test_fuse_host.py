"""The point-cloud export on the CPU: the numpy restatement of the rule (tests/fuse_reference.py) on the analytic scene, the decision
margins that let a GPU test ask for exact equality, the PLY writer, the camera table, the header group of the binding and the
native program's fixture."""
import collections
import ctypes
import os
import shutil
import subprocess

import numpy
import pytest

from simplenerf_amd import _lib, build, geometry

from . import fuse_reference as ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARGIN = 1e-9                       # a decision closer than this to its threshold (relative to d_u) or to a rounding tie may be left out
KEPT = {1: (577, (178, 221, 178)), 2: (372, (120, 124, 128))}     # min_views -> (kept, kept per view), the same for both tau


def test_fuse_header_is_the_bindings_next_group():
    assert [os.path.relpath(path, REPO) for path in _lib.FUSE_HEADERS] == [os.path.join('simplenerf_amd', 'csrc', 'simplenerf_fuse.h')]
    assert set(_lib.FUSE_SIGNATURES) == {'snerf_fuse_depth_maps_workspace_bytes', 'snerf_fuse_depth_maps', 'snerf_voxel_thin_workspace_bytes',
                                         'snerf_voxel_thin'}
    earlier = set(_lib.SIGNATURES) | set(_lib.ADDED_SIGNATURES) | set(_lib.SWEEP_SIGNATURES) | set(_lib.SWEEP16_SIGNATURES) \
        | set(_lib.PNG_SIGNATURES) | set(_lib.JPEG_SIGNATURES)
    assert not earlier & set(_lib.FUSE_SIGNATURES)
    assert _lib.FUSE_SIGNATURES['snerf_fuse_depth_maps_workspace_bytes'] == (ctypes.c_longlong, [ctypes.c_int] * 3)
    assert _lib.FUSE_SIGNATURES['snerf_voxel_thin_workspace_bytes'] == (ctypes.c_longlong, [ctypes.c_longlong] + [ctypes.c_int] * 3)
    restype, argtypes = _lib.FUSE_SIGNATURES['snerf_fuse_depth_maps']
    assert restype is ctypes.c_int and argtypes == [ctypes.c_void_p] * 4 + [ctypes.c_int] * 3 + [ctypes.c_double, ctypes.c_int] \
        + [ctypes.c_void_p] * 6
    restype, argtypes = _lib.FUSE_SIGNATURES['snerf_voxel_thin']
    assert restype is ctypes.c_int and argtypes == [ctypes.c_void_p] * 2 + [ctypes.c_longlong] + [ctypes.c_double] * 4 + [ctypes.c_int] * 3 \
        + [ctypes.c_void_p] * 6
    assert _lib.C.SNERF_FUSE_CAMERA_DOUBLES == 42 and _lib.C.SNERF_FUSE_MAX_VIEWS == 255 and _lib.ABI_VERSION == 10


@pytest.mark.parametrize('tau', [0.02, 0.05])
@pytest.mark.parametrize('min_views', [1, 2])
def test_restatement_on_the_scene_gives_the_pinned_counts(tau, min_views):
    scene = ref.scene()
    assert scene['depth'].shape == (3, 13, 17) and scene['depth'].dtype == numpy.float32
    points, colours, views, sources, margins = ref.scene_expected(tau, min_views)
    assert len(margins) == 663                                     # every pixel of the scene is valid
    per_view = collections.Counter(sources[:, 0].tolist())
    assert (len(points), tuple(per_view[v] for v in range(3))) == KEPT[min_views]
    assert points.dtype == numpy.float32 and colours.dtype == numpy.uint8 and views.dtype == numpy.uint8
    assert views.min() >= min_views and views.max() <= 2
    assert numpy.array_equal(colours, scene['image'][sources[:, 0], sources[:, 1], sources[:, 2]])
    assert [tuple(s) for s in sources.tolist()] == sorted(tuple(s) for s in sources.tolist())     # ascending (v, y, x)


@pytest.mark.parametrize('tau', [0.02, 0.05])
def test_no_decision_of_the_scene_is_marginal(tau):
    """The condition under which the GPU test may ask for the exact kept set: pixels decided within 1e-9 may be left out, at most 1 %
    of the valid ones.  On this scene there are none: the closest threshold decision is 0.0194 (tau = 0.02) or 0.0494 (tau = 0.05)
    away over 1192 lookups, the closest rounding tie 0.0034."""
    margins = ref.scene_expected(tau, 1)[4]
    marginal = [key for key, m in margins.items() if m['threshold'] < MARGIN or m['tie'] < MARGIN]
    assert len(marginal) <= 0.01 * len(margins)
    assert sum(m['lookups'] for m in margins.values()) == 1192
    closest = min(m['threshold'] for m in margins.values())
    assert abs(closest - (tau - 0.0006)) < 1e-4, closest
    assert abs(min(m['tie'] for m in margins.values()) - 0.0034) < 1e-4
    assert marginal == []


def test_kept_points_lie_on_the_planes():
    """Every kept pixel's point is on the plane z = 5 or z = 10: to 1e-9 from the scene's depths as computed (float64), which holds the
    restated geometry -- cameras, pixel convention, unprojection -- to the analytic scene; the depth MAPS are those depths rounded
    to float32, half an ulp of 10 (4.8e-7) at the most, so the restated points themselves are held to that rounding (measured:
    4.8e-7) plus their own cast to float32 (another 4.8e-7)."""
    scene = ref.scene()
    points, _, _, sources, _ = ref.scene_expected(0.02, 1)
    e_inv = [numpy.linalg.inv(m) for m in scene['extrinsics']]
    k_inv = [numpy.linalg.inv(m) for m in scene['intrinsics']]
    on_near = 0
    for point, (v, y, x) in zip(points, sources.tolist()):
        exact = ref.point_of(e_inv[v], k_inv[v], x, y, scene['depth64'][v, y, x])
        off = min(abs(exact[2] - ref.NEAR_PLANE), abs(exact[2] - ref.FAR_PLANE))
        assert off <= 1e-9, (v, y, x, exact)
        if abs(exact[2] - ref.NEAR_PLANE) <= 1e-9:
            on_near += 1
            assert abs(exact[0]) <= ref.NEAR_HALF_SIDE + 1e-9 and abs(exact[1]) <= ref.NEAR_HALF_SIDE + 1e-9
        assert numpy.abs(point.astype(numpy.float64) - exact).max() <= 2.0 ** -24 * 10.0 * 2, (v, y, x)
    assert 0 < on_near < len(points)                               # both planes are seen


def test_ply_bytes_parse_back():
    points, colours = ref.scene_expected(0.02, 1)[:2]
    data = geometry.ply_bytes(points, colours)
    header = (b'ply\nformat binary_little_endian 1.0\nelement vertex 577\nproperty float x\nproperty float y\nproperty float z\n'
              b'property uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n')
    assert data.startswith(header) and len(data) == len(header) + 577 * 15
    vertex = numpy.dtype([('x', '<f4'), ('y', '<f4'), ('z', '<f4'), ('red', 'u1'), ('green', 'u1'), ('blue', 'u1')])
    assert vertex.itemsize == 15
    records = numpy.frombuffer(data[len(header):], dtype=vertex)
    assert numpy.array_equal(numpy.stack([records['x'], records['y'], records['z']], axis=1).view(numpy.uint32), points.view(numpy.uint32))
    assert numpy.array_equal(numpy.stack([records['red'], records['green'], records['blue']], axis=1), colours)
    empty = geometry.ply_bytes(numpy.zeros((0, 3), numpy.float32), numpy.zeros((0, 3), numpy.uint8))
    assert empty == header.replace(b'vertex 577', b'vertex 0')      # N = 0 is a valid file
    with pytest.raises(RuntimeError, match='points'):
        geometry.ply_bytes(points.astype(numpy.float64), colours)
    with pytest.raises(RuntimeError, match='colours'):
        geometry.ply_bytes(points, colours[:-1])


def test_save_ply_leaves_an_existing_file_alone(tmp_path):
    points, colours = ref.scene_expected(0.02, 2)[:2]
    path = tmp_path / 'clouds' / 'scene.ply'
    geometry.save_ply(path, points, colours)
    assert path.read_bytes() == geometry.ply_bytes(points, colours)
    geometry.save_ply(path, points[:3], colours[:3])
    assert path.read_bytes() == geometry.ply_bytes(points, colours)


def test_fuse_cameras_table():
    scene = ref.scene()
    table = geometry.fuse_cameras(scene['extrinsics'], scene['intrinsics'].astype(numpy.float32))
    assert table.shape == (3, 42) and table.dtype == numpy.float64
    for v in range(3):
        assert numpy.array_equal(table[v, 0:9].reshape(3, 3), numpy.linalg.inv(scene['intrinsics'][v]))
        assert numpy.array_equal(table[v, 9:21].reshape(3, 4), numpy.linalg.inv(scene['extrinsics'][v])[:3])
        assert numpy.array_equal(table[v, 21:33].reshape(3, 4), scene['extrinsics'][v][:3])
        assert numpy.array_equal(table[v, 33:42].reshape(3, 3), scene['intrinsics'][v])
    with pytest.raises(RuntimeError, match='intrinsics'):
        geometry.fuse_cameras(scene['extrinsics'], scene['intrinsics'][:2])


def test_camera_matrices_turn_the_pose_round():
    """pose: camera-to-world, looking down -z, y up.  A pixel right of and below the principal point lies at +x, -y, -z of the pose's
    axes, at z-depth t."""
    pose = numpy.eye(4)
    pose[:3, 3] = (0.5, -1.0, 2.0)
    camera = {'pose': pose.astype(numpy.float32), 'intrinsic': numpy.array([[10.0, 0, 3], [0, 10.0, 2], [0, 0, 1]], numpy.float32)}
    extrinsic, intrinsic = geometry.camera_matrices(camera)
    assert extrinsic.dtype == numpy.float64 and intrinsic.dtype == numpy.float64
    point = numpy.matmul(numpy.linalg.inv(extrinsic)[:3], numpy.append(4.0 * numpy.matmul(numpy.linalg.inv(intrinsic), [5.0, 3.0, 1.0]), 1.0))
    assert numpy.allclose(point, [0.5 + 0.8, -1.0 - 0.4, 2.0 - 4.0], atol=1e-12)


def test_thinning_restatement_on_a_hand_made_case():
    """Voxels of side 1 from (0, 0, 0): three points in voxel (0, 0, 0), one in (1, 0, 0), two in (0, 1, 1); keys 0, 1, 2 + 2 * 2."""
    points = numpy.array([[0.0, 0.0, 0.0], [1.5, 0.25, 0.5], [0.5, 1.5, 1.0], [0.25, 0.5, 0.75], [0.75, 1.0, 1.5], [0.5, 0.25, 0.25]],
                         dtype=numpy.float32)
    colours = numpy.array([[0, 10, 255], [7, 8, 9], [100, 0, 1], [1, 11, 255], [101, 1, 2], [1, 12, 254]], dtype=numpy.uint8)
    lo, extents = ref.voxel_grid(points, 1.0)
    assert lo.tolist() == [0.0, 0.0, 0.0] and extents == (2, 2, 2)
    thinned, thinned_colours, counts = ref.voxel_thin(points, colours, 1.0)
    assert counts.tolist() == [3, 1, 2] and counts.dtype == numpy.int32
    assert thinned.tolist() == [[0.25, 0.25, numpy.float32(1.0 / 3.0)], [1.5, 0.25, 0.5], [0.625, 1.25, 1.25]]
    # (2 * sum + count) div (2 * count): 2/3 -> 1, 33/3 = 11, 764/3 = 254.67 -> 255; 201/2 = 100.5 -> 101, 1/2 -> 1, 3/2 -> 2
    assert thinned_colours.tolist() == [[1, 11, 255], [7, 8, 9], [101, 1, 2]]
    # a sequential sum is not numpy's pairwise one: the restatement must keep the order of the rule
    many = numpy.full((4096, 3), 0.1, dtype=numpy.float32)
    many[0] = 1e8
    many[-1] = -1e8 + 64
    mean = ref.voxel_thin(many, numpy.zeros((4096, 3), numpy.uint8), 1e9)[0]
    total = 0.0
    for value in many[:, 0]:
        total += float(value)
    assert mean.shape == (1, 3) and mean[0, 0] == numpy.float32(total / 4096)
    empty = ref.voxel_thin(numpy.zeros((0, 3), numpy.float32), numpy.zeros((0, 3), numpy.uint8), 1.0)
    assert [len(a) for a in empty] == [0, 0, 0]


def test_native_fixture_layout():
    data = ref.native_fixture()
    views, h, w, min_views = numpy.frombuffer(data[:16], '<i4').tolist()
    assert (views, h, w, min_views) == (3, 13, 17, ref.NATIVE_MIN_VIEWS)
    n, m = 577, len(ref.voxel_thin(*ref.scene_expected(ref.NATIVE_TAU, ref.NATIVE_MIN_VIEWS)[:2], ref.NATIVE_VOXEL)[0])
    total = views * h * w
    assert len(data) == 16 + 8 + views * 42 * 8 + total * 4 + total * 3 + 8 + n * 16 + 8 * 4 + 3 * 4 + 8 + m * 19
    at = 24 + views * 42 * 8 + total * 7
    assert int(numpy.frombuffer(data[at:at + 8], '<i8')[0]) == n


@pytest.mark.skipif(shutil.which(build.HIPCC) is None and not os.path.exists(build.HIPCC), reason='hipcc not available')
def test_fuse_abi_program_compiles_and_links(tmp_path):
    """CPU-side half of the native smoke: the new header is valid C++ for an outside consumer and the four symbols link."""
    build.build_library()
    assert os.path.exists(compile_smoke(str(tmp_path)))


def compile_smoke(out_dir):
    exe = os.path.join(out_dir, 'fuse_abi_smoke')
    lib_dir = os.path.dirname(_lib.LIB_PATH)
    cmd = [build.HIPCC, '--offload-arch=gfx950', '-O1', '-std=c++17', f'-I{os.path.join(REPO, "include")}', f'-I{build.CSRC}',
           os.path.join(REPO, 'tests', 'native', 'fuse_abi_smoke.cpp'), '-o', exe, f'-L{lib_dir}', '-lsimplenerf_hip',
           f'-Wl,-rpath,{lib_dir}']
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe
