"""Normal maps on the CPU: the eleventh header group of the binding, the PLY point cloud with normals, the refusals that need no
device, the restatement of tests/normals_reference.py checked against itself three ways (the inverse input map against the forward
one of tests/field_reference.py, a planar slab, a fronto-parallel plane), and the native program.  The cases the GPU tests share
(tests/test_gpu_normals.py) are built here, once."""
import ctypes
import functools
import math
import os
import shutil
import struct
import subprocess

import numpy
import pytest
import torch

from simplenerf_amd import _lib, build, geometry, harness, ops

from . import field_reference, mesh_reference
from . import normals_reference as nref
from .test_field_gradient_host import test_gradient_header_is_the_bindings_tenth_group as gradient_group_is_unchanged

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HAS_HIPCC = shutil.which(build.HIPCC) is not None or os.path.exists(build.HIPCC)
U = 2.0 ** -53            # the relative error of one correctly rounded fp64 operation


def _frozen(*arrays):
    for array in arrays:
        array.setflags(write=False)
    return arrays


# ------------------------------------------------------------------------------------------------------------------ the shared cases
SELECTION_RAYS = (1, 63, 64, 65, 257, 1000)
SELECTION_SAMPLES = (1, 2, 7, 64, 65, 192)
SELECTION_WIDE = (5000, 7)          # 5001 counts: the in-place scan of the offsets takes three chunks of 2048


@functools.lru_cache(maxsize=None)
def selection_case(rays, samples):
    """(origins, dirs, z_vals, weights) float32: weights in [0, 1) with runs of exact zeros, every fifth ray all zero, every
    seventh all at least 0.5, and one NaN."""
    rng = numpy.random.default_rng(1000 * rays + samples)
    origins = rng.standard_normal((rays, 3)).astype(numpy.float32)
    dirs = rng.standard_normal((rays, 3)).astype(numpy.float32)
    z_vals = numpy.sort(rng.uniform(0.0, 6.0, (rays, samples)), axis=1).astype(numpy.float32)
    weights = rng.uniform(0.0, 1.0, (rays, samples)).astype(numpy.float32)
    flat = weights.reshape(-1)
    for _ in range(max(1, flat.size // 40)):                       # runs of exact zeros, across ray boundaries too
        first = int(rng.integers(0, flat.size))
        flat[first:first + int(rng.integers(1, 70))] = 0.0
    weights[4::5] = 0.0
    weights[6::7] = rng.uniform(0.5, 1.0, weights[6::7].shape).astype(numpy.float32)
    weights[rays // 2, samples // 3] = numpy.nan
    return _frozen(origins, dirs, z_vals, weights)


@functools.lru_cache(maxsize=None)
def composite_case(with_ndc):
    """(points, grad, offsets, sample, weights, ndc): 300 rays of 16 samples selected at 0.25, with random gradients of every
    magnitude, exact zeros, +-inf and NaN; with ndc the points' z lies on both sides of -1 and of 1."""
    rng = numpy.random.default_rng(21 + int(with_ndc))
    rays, samples = 300, 16
    weights = rng.uniform(0.0, 1.0, (rays, samples)).astype(numpy.float32)
    weights[3] = 0.0
    weights[7, 5] = numpy.nan
    zeros = numpy.zeros((rays, 3), dtype=numpy.float32)
    offsets, sample, _ = nref.select_ray_samples(zeros, zeros, numpy.zeros((rays, samples), numpy.float32), weights, 0.25)
    count = len(sample)
    points = rng.uniform(-1.5, 1.5, (count, 3)).astype(numpy.float32)
    points[10, 2], points[11, 2], points[12, 2], points[13, 2] = 1.0, -1.0, numpy.nan, numpy.float32(1.0) - numpy.float32(2.0 ** -24)
    grad = (rng.standard_normal((count, 3)) * 10.0 ** rng.uniform(-3, 3, (count, 1))).astype(numpy.float32)
    grad[::11] = 0.0
    grad[20], grad[21], grad[22] = [numpy.inf, 1.0, 0.0], [1.0, -numpy.inf, 2.0], [numpy.nan, 1.0, 0.0]
    grad[23] = [3.0e38, 3.0e38, 0.0]                               # finite in fp64
    first = int(offsets[40])
    grad[first:int(offsets[41])] = 0.0                             # a ray whose every selected sample has no gradient
    ndc = field_reference.fern_cameras()[2] if with_ndc else None
    return _frozen(points, grad, offsets, sample, weights) + (ndc,)


# the planar slab: density k max(0, a . x - b) = max(0, g . x - c) with g = k a a float32 vector and c = k b
SLAB_GRADIENT = numpy.array([12.0, -9.0, 20.0], dtype=numpy.float32)
SLAB_OFFSET = 30.0
SLAB_RAYS, SLAB_SAMPLES = 130, 40


def slab_normal():
    g = SLAB_GRADIENT.astype(numpy.float64)
    return -g / math.sqrt(float((g * g).sum()))


@functools.lru_cache(maxsize=None)
def slab_case():
    """(origins, dirs, z_vals, weights float32, points float32 (R,S,3), inside bool (R,S)): rays from near the origin, most of them
    into the half-space g . x > c, the rest away from it; the weights are alpha-composited in float64 from the density at the
    float32 points the selection forms."""
    rng = numpy.random.default_rng(5)
    origins = (0.1 * rng.standard_normal((SLAB_RAYS, 3))).astype(numpy.float32)
    towards = -slab_normal()
    dirs = towards[None] + 0.4 * rng.standard_normal((SLAB_RAYS, 3))
    dirs[::6] = -dirs[::6]                                          # these rays leave: they miss the slab
    dirs = (dirs / numpy.linalg.norm(dirs, axis=1, keepdims=True)).astype(numpy.float32)
    z_vals = numpy.broadcast_to(numpy.linspace(0.25, 4.0, SLAB_SAMPLES, dtype=numpy.float32), (SLAB_RAYS, SLAB_SAMPLES)).copy()
    points = origins[:, None, :] + dirs[:, None, :] * z_vals[:, :, None]             # float32: product, then sum
    assert points.dtype == numpy.float32
    height = points.astype(numpy.float64) @ SLAB_GRADIENT.astype(numpy.float64) - SLAB_OFFSET
    sigma = numpy.maximum(0.0, height)
    delta = numpy.diff(z_vals.astype(numpy.float64), axis=1, append=1e10) * numpy.linalg.norm(dirs.astype(numpy.float64), axis=1, keepdims=True)
    alpha = 1.0 - numpy.exp(-sigma * delta)
    through = numpy.cumprod(numpy.concatenate([numpy.ones((SLAB_RAYS, 1)), 1.0 - alpha + 1e-10], axis=1), axis=1)[:, :-1]
    weights = (alpha * through).astype(numpy.float32)
    return _frozen(origins, dirs, z_vals, weights, points, height > 0.0)


def slab_gradient(points):
    """The slab's density gradient at float32 (n,3) points, as a float32 array: g inside, 0 outside."""
    inside = points.astype(numpy.float64) @ SLAB_GRADIENT.astype(numpy.float64) - SLAB_OFFSET > 0.0
    return numpy.where(inside[:, None], SLAB_GRADIENT[None], numpy.float32(0.0)).astype(numpy.float32)


DEPTH_FRAMES = ((1, 1), (1, 5), (5, 1), (3, 4), (17, 33), (64, 65))


def pinhole(height, width, focal):
    return numpy.array([[focal, 0.0, width / 2.0], [0.0, focal, height / 2.0], [0.0, 0.0, 1.0]])


@functools.lru_cache(maxsize=None)
def depth_case(views, height, width):
    """(depth float32 (V,h,w), mask uint8 (V,h,w), cameras float64 (V,42), extrinsics, intrinsics): a wavy surface with steps, seen by
    slightly turned cameras, with holes of every kind -- 0, negative, NaN, inf and the mask."""
    rng = numpy.random.default_rng(100 * views + 10 * height + width)
    y, x = numpy.mgrid[0:height, 0:width]
    extrinsics, intrinsics, depth = [], [], []
    for v in range(views):
        pose = mesh_reference.look_at((0.3 * v - 0.2, 0.1 * v, -3.0 - 0.2 * v))
        extrinsics.append(numpy.asarray(pose, dtype=numpy.float64).reshape(4, 4))
        intrinsics.append(pinhole(height, width, 0.9 * max(height, width)))
        surface = 3.0 + 0.3 * numpy.sin(0.7 * x + v) + 0.2 * numpy.cos(0.5 * y) + 0.8 * ((x + 2 * y) % 11 > 7)
        depth.append(surface + 0.01 * rng.standard_normal((height, width)))
    depth = numpy.stack(depth).astype(numpy.float32)
    flat = depth.reshape(-1)
    holes = rng.permutation(flat.size)
    if flat.size >= 20:
        for kind, value in enumerate((0.0, -1.5, numpy.nan, numpy.inf)):
            flat[holes[kind::9][:max(1, flat.size // 25)]] = value
    mask = numpy.ones(depth.shape, dtype=numpy.uint8)
    if flat.size >= 20:
        mask.reshape(-1)[holes[4::9][:max(1, flat.size // 25)]] = 0
    cameras = geometry.fuse_cameras(numpy.stack(extrinsics), numpy.stack(intrinsics))
    return _frozen(depth, mask, cameras) + (extrinsics, intrinsics)


def fronto_parallel_case(height=9, width=12, distance=2.5):
    """(depth, cameras): a plane at an exactly representable depth before an identity pose, power-of-two focal length and centre."""
    depth = numpy.full((1, height, width), distance, dtype=numpy.float32)
    intrinsic = numpy.array([[16.0, 0.0, 8.0], [0.0, 16.0, 4.0], [0.0, 0.0, 1.0]])
    return depth, geometry.fuse_cameras(numpy.eye(4)[None], intrinsic[None])


OBLIQUE_NORMAL = numpy.array([0.36, -0.48, -0.8])          # a unit vector; the plane is n . X = OBLIQUE_OFFSET
OBLIQUE_OFFSET = -2.4


def oblique_plane_case(height=17, width=33):
    """(depth float32 (1,h,w), cameras, bound (h,w)): the plane OBLIQUE_NORMAL . X = OBLIQUE_OFFSET before an identity pose, its
    depth rounded to float32, and per pixel the bound on |normal - OBLIQUE_NORMAL| derived in
    tests/test_gpu_normals.py::test_an_oblique_planes_normals_are_within_the_depth_roundings_reach."""
    intrinsic = pinhole(height, width, 40.0)
    inverse = numpy.linalg.inv(intrinsic)
    y, x = numpy.mgrid[0:height, 0:width]
    rays = numpy.stack([x, y, numpy.ones_like(x)], axis=-1).astype(numpy.float64) @ inverse.T             # (h,w,3), z = 1
    exact = OBLIQUE_OFFSET / (rays @ OBLIQUE_NORMAL)
    assert (exact > 0).all()
    points = exact[..., None] * rays
    farthest = float(numpy.linalg.norm(points, axis=-1).max())
    bound = numpy.zeros((height, width))
    for j in range(height):
        for i in range(width):
            left, right, up, down = max(i - 1, 0), min(i + 1, width - 1), max(j - 1, 0), min(j + 1, height - 1)
            tx, ty = points[j, right] - points[j, left], points[down, i] - points[up, i]
            cross = float(numpy.linalg.norm(numpy.cross(tx, ty)))
            reach = 2.0 ** -23 * farthest * (float(numpy.linalg.norm(tx)) + float(numpy.linalg.norm(ty))) + (2.0 ** -23 * farthest) ** 2
            bound[j, i] = 2.0 * reach / cross + 2.0 ** -23
    cameras = geometry.fuse_cameras(numpy.eye(4)[None], intrinsic[None])
    return exact[None].astype(numpy.float32), cameras, bound


def picture_case():
    """(normals float32 (N,3), rotation (3,3)): unit normals, zeros, NaN, components of +-1, lengths above 1."""
    rng = numpy.random.default_rng(8)
    normals = rng.standard_normal((500, 3))
    normals = (normals / numpy.linalg.norm(normals, axis=1, keepdims=True)).astype(numpy.float32)
    normals[:6] = [[0, 0, 0], [1, 0, 0], [0, -1, 0], [0, 0, 1], [-1, -1, -1], [1, 1, 1]]
    normals[6] = [numpy.nan, 0.5, -0.5]
    normals[7] = [numpy.inf, -numpy.inf, 3.0]
    normals[8] = [-0.0, 1e-9, -1e-9]
    rotation = numpy.asarray(field_reference.fern_cameras()[0][1]['pose'], dtype=numpy.float64).reshape(4, 4)[:3, :3]
    return normals, rotation


# ------------------------------------------------------------------------------------------------------------------ ABI and binding
def test_normals_header_is_the_bindings_eleventh_group():
    assert [os.path.relpath(path, REPO) for path in _lib.NORMALS_HEADERS] == [os.path.join('simplenerf_amd', 'csrc', 'simplenerf_normals.h')]
    assert set(_lib.NORMALS_SIGNATURES) == {'snerf_ray_samples_count', 'snerf_ray_samples_emit', 'snerf_composite_normals',
                                            'snerf_depth_normals', 'snerf_normals_to_u8'}
    earlier = set(_lib.SIGNATURES) | set(_lib.ADDED_SIGNATURES) | set(_lib.SWEEP_SIGNATURES) | set(_lib.SWEEP16_SIGNATURES) \
        | set(_lib.PNG_SIGNATURES) | set(_lib.JPEG_SIGNATURES) | set(_lib.FUSE_SIGNATURES) | set(_lib.MESH_SIGNATURES) \
        | set(_lib.FIELD_SIGNATURES) | set(_lib.GRADIENT_SIGNATURES)
    assert not earlier & set(_lib.NORMALS_SIGNATURES)
    p, ll, i, d = ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int, ctypes.c_double
    assert _lib.NORMALS_SIGNATURES['snerf_ray_samples_count'] == (i, [p, ll, i, d, p, p])
    assert _lib.NORMALS_SIGNATURES['snerf_ray_samples_emit'] == (i, [p, p, p, p, ll, i, d, p, ll, p, p, p])
    assert _lib.NORMALS_SIGNATURES['snerf_composite_normals'] == (i, [p, p, ll, p, p, p, ll, i, i, d, d, d, p, p, p])
    assert _lib.NORMALS_SIGNATURES['snerf_depth_normals'] == (i, [p, p, p, i, i, i, d, p, p])
    assert _lib.NORMALS_SIGNATURES['snerf_normals_to_u8'] == (i, [p, ll, p, p, p])
    assert _lib.ABI_VERSION == 10
    gradient_group_is_unchanged()


@pytest.mark.skipif(not HAS_HIPCC, reason='hipcc not available')
def test_normals_symbols_are_exported():
    build.build_library()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in _lib.NORMALS_SIGNATURES:
        assert hasattr(lib, name), name


@pytest.mark.skipif(not HAS_HIPCC, reason='hipcc not available')
def test_the_librarys_refusals_come_before_any_launch():
    """Every check is made on the host before the first launch, so the status codes need no device."""
    build.build_library()
    lib = _lib.load()
    invalid, unsupported = _lib.C.SNERF_E_INVALID, _lib.C.SNERF_E_UNSUPPORTED
    here = ctypes.c_void_p(256)             # a non-NULL pointer that is never followed: every call below is refused first
    assert lib.snerf_ray_samples_count(here, -1, 4, 0.0, here, None) == invalid
    assert lib.snerf_ray_samples_count(here, 4, -1, 0.0, here, None) == invalid
    assert lib.snerf_ray_samples_count(here, 4, 4, math.nan, here, None) == invalid
    assert lib.snerf_ray_samples_count(here, 4, 4, 0.0, None, None) == invalid
    assert lib.snerf_ray_samples_count(None, 4, 4, 0.0, here, None) == invalid
    assert lib.snerf_ray_samples_count(here, 1 << 20, 1 << 11, 0.0, here, None) == unsupported
    assert b'num_rays . num_samples' in lib.snerf_last_error() and b'2^31 - 1' in lib.snerf_last_error()
    assert lib.snerf_ray_samples_emit(here, here, here, here, 1 << 20, 1 << 11, 0.0, here, 5, here, here, None) == unsupported
    assert b'num_rays . num_samples' in lib.snerf_last_error()
    assert lib.snerf_ray_samples_emit(here, here, here, here, 4, 4, 0.0, here, -1, here, here, None) == invalid
    assert lib.snerf_ray_samples_emit(here, here, here, here, 4, 4, 0.0, here, 5, None, here, None) == invalid
    assert lib.snerf_ray_samples_emit(here, here, here, here, 4, 4, 0.0, None, 5, here, here, None) == invalid
    assert lib.snerf_ray_samples_emit(None, None, None, None, 0, 4, 0.0, here, 0, None, None, None) == 0        # nothing to emit
    assert lib.snerf_ray_samples_emit(here, here, here, here, 4, 4, 0.0, here, 0, None, None, None) == 0
    composite = lambda count, rays, samples, ndc, normal=here: lib.snerf_composite_normals(
        here, here, count, here, here, here, rays, samples, *ndc, normal, here, None)
    assert composite(-1, 4, 4, (0, 0.0, 0.0, 0.0)) == invalid
    assert composite(5, -4, 4, (0, 0.0, 0.0, 0.0)) == invalid
    assert composite(5, 4, 4, (1, 1.0, 1.0, 0.0)) == invalid and b'near' in lib.snerf_last_error()
    assert composite(5, 4, 4, (1, math.inf, 1.0, 1.0)) == invalid
    assert composite(5, 4, 4, (0, 0.0, 0.0, 0.0), None) == invalid
    assert composite(1 << 31, 4, 4, (0, 0.0, 0.0, 0.0)) == unsupported
    assert composite(5, 1 << 20, 1 << 11, (0, 0.0, 0.0, 0.0)) == unsupported
    assert composite(0, 0, 4, (0, 0.0, 0.0, 0.0), None) == 0
    assert lib.snerf_depth_normals(here, None, here, -1, 4, 4, -1.0, here, None) == invalid
    assert lib.snerf_depth_normals(here, None, here, 256, 4, 4, -1.0, here, None) == invalid
    assert lib.snerf_depth_normals(here, None, here, 2, 4, 4, math.nan, here, None) == invalid
    assert lib.snerf_depth_normals(here, None, None, 2, 4, 4, -1.0, here, None) == invalid
    assert lib.snerf_depth_normals(here, None, here, 2, 1 << 16, 1 << 15, -1.0, here, None) == unsupported
    assert lib.snerf_depth_normals(None, None, None, 2, 0, 4, -1.0, None, None) == 0
    rotation = (ctypes.c_double * 9)(1, 0, 0, 0, 1, 0, 0, 0, math.nan)
    assert lib.snerf_normals_to_u8(here, 4, rotation, here, None) == invalid and b'rotation[8]' in lib.snerf_last_error()
    assert lib.snerf_normals_to_u8(here, -4, None, here, None) == invalid
    assert lib.snerf_normals_to_u8(None, 4, None, here, None) == invalid
    assert lib.snerf_normals_to_u8(here, 1 << 31, None, here, None) == unsupported
    assert lib.snerf_normals_to_u8(None, 0, None, None, None) == 0


def test_python_refusals_without_a_device():
    host = torch.zeros((4, 3))
    with pytest.raises(RuntimeError, match='weights.*GPU'):
        ops.select_ray_samples(host, host, torch.zeros((4, 2)), torch.zeros((4, 2)))
    with pytest.raises(RuntimeError, match='weights.*GPU'):
        ops.composite_normals(host, host, torch.zeros(5, dtype=torch.int32), torch.zeros(4, dtype=torch.int32), torch.zeros((4, 2)))
    with pytest.raises(RuntimeError, match='depth.*GPU'):
        ops.depth_normals(torch.zeros((1, 4, 4)), torch.zeros((1, 42), dtype=torch.float64))
    with pytest.raises(RuntimeError, match='normals.*GPU'):
        ops.normals_to_u8(host)
    with pytest.raises(RuntimeError, match='GPU'):
        geometry.ray_normals(lambda p: p, host, host, torch.zeros((4, 2)), torch.zeros((4, 2)))
    with pytest.raises(RuntimeError, match='GPU'):
        geometry.depth_normals(torch.zeros((1, 4, 4)), numpy.eye(4)[None], numpy.eye(3)[None])
    with pytest.raises(RuntimeError, match='GPU'):
        geometry.normals_to_u8(host)
    # a model whose gradient does not exist is refused before anything else is looked at
    from simplenerf_amd import synth
    from simplenerf_amd.models.ModelFactory import get_model
    camera = synth.camera('fern', 0, resolution=(8, 6))
    for overrides, word in ((dict(predict_visibility=True), 'predict_visibility'),
                            (dict(points_net_depth=6, points_net_width=96, views_net_width=48), 'layered')):
        cfg = synth.make_configs('config1')
        cfg['model']['coarse_mlp'].update(overrides)
        model = get_model(cfg, None)
        if not HAS_HIPCC and word == 'layered':
            continue                       # (the descriptor's check is the library's)
        with pytest.raises(NotImplementedError, match=word):
            harness.predict_normals(model, cfg, camera, 'cpu')
        with pytest.raises(NotImplementedError, match=word):
            harness.export_point_cloud(model, cfg, [camera], 'never.ply', 'cpu', normals=True)
        with pytest.raises(NotImplementedError, match=word):
            harness.export_mesh(model, cfg, [camera], 'never.ply', 'cpu', 0.1, normals=True)
    assert not os.path.exists('never.ply')


# ------------------------------------------------------------------------------------------------------------------ the PLY
def todays_ply_bytes(points, colours):
    """The point-cloud file before normals existed, written out again from the format's own words."""
    header = ('ply\nformat binary_little_endian 1.0\n' + f'element vertex {len(points)}\nproperty float x\nproperty float y\nproperty float z\n'
              + 'property uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n').encode('ascii')
    return header + b''.join(numpy.asarray(p, '<f4').tobytes() + numpy.asarray(c, 'u1').tobytes() for p, c in zip(points, colours))


def parse_ply_with_normals(data):
    header, body = data.split(b'end_header\n', 1)
    lines = header.decode('ascii').split('\n')
    assert lines[:2] == ['ply', 'format binary_little_endian 1.0'] and len(lines) == 13 and lines[-1] == ''
    assert lines[3:12] == [f'property float {a}' for a in ('x', 'y', 'z', 'nx', 'ny', 'nz')] + [f'property uchar {c}' for c in ('red', 'green', 'blue')]
    count = int(lines[2].split()[-1])
    assert lines[2] == f'element vertex {count}' and len(body) == 27 * count
    return numpy.frombuffer(body, dtype=geometry.PLY_VERTEX_NORMAL)


def test_ply_point_cloud_with_normals_and_without(tmp_path):
    rng = numpy.random.default_rng(4)
    points = rng.standard_normal((9, 3)).astype(numpy.float32)
    normals = rng.standard_normal((9, 3)).astype(numpy.float32)
    colours = rng.integers(0, 256, (9, 3)).astype(numpy.uint8)
    plain = geometry.ply_bytes(points, colours)
    assert plain == todays_ply_bytes(points, colours) == geometry.ply_bytes(points, colours, None)
    data = geometry.ply_bytes(torch.from_numpy(points), colours, torch.from_numpy(normals))
    assert geometry.PLY_VERTEX_NORMAL.itemsize == 27
    assert len(data) - len(plain) == 9 * 12 + len(b'property float nx\nproperty float ny\nproperty float nz\n')
    records = parse_ply_with_normals(data)
    assert numpy.array_equal(numpy.stack([records[k] for k in ('x', 'y', 'z')], axis=1), points)
    assert numpy.array_equal(numpy.stack([records[k] for k in ('nx', 'ny', 'nz')], axis=1), normals)
    assert numpy.array_equal(numpy.stack([records[k] for k in ('red', 'green', 'blue')], axis=1), colours)
    assert parse_ply_with_normals(geometry.ply_bytes(points[:0], colours[:0], normals[:0])).shape == (0,)
    # the mesh writer's vertex element is this one
    triangles = rng.integers(0, 9, (4, 3)).astype(numpy.int32)
    mesh = geometry.ply_mesh_bytes(points, colours, triangles, normals)
    assert mesh.split(b'end_header\n', 1)[1][:27 * 9] == data.split(b'end_header\n', 1)[1]
    geometry.save_ply(tmp_path / 'a.ply', points, colours, normals)
    geometry.save_ply(tmp_path / 'b.ply', points, colours)
    assert (tmp_path / 'a.ply').read_bytes() == data and (tmp_path / 'b.ply').read_bytes() == plain
    geometry.save_ply(tmp_path / 'a.ply', points, colours)                       # an existing file is left alone
    assert (tmp_path / 'a.ply').read_bytes() == data
    for bad in (normals[:8], normals.astype(numpy.float64), normals[:, :2]):
        with pytest.raises(RuntimeError, match='normals'):
            geometry.ply_bytes(points, colours, bad)


# ------------------------------------------------------------------------------------------------------------------ the restatement
def test_selection_restated_on_a_case_done_by_hand():
    origins = numpy.array([[1.0, 2.0, 3.0], [0.0, 0.0, 0.0]], dtype=numpy.float32)
    dirs = numpy.array([[0.5, -1.0, 0.25], [1.0, 1.0, 1.0]], dtype=numpy.float32)
    z_vals = numpy.array([[1.0, 2.0, 4.0], [0.1, 0.2, 0.3]], dtype=numpy.float32)
    weights = numpy.array([[0.0, 0.5, 0.25], [numpy.nan, 0.0, 1.0]], dtype=numpy.float32)
    offsets, sample, points = nref.select_ray_samples(origins, dirs, z_vals, weights)
    assert offsets.tolist() == [0, 2, 3] and sample.tolist() == [1, 2, 5] and offsets.dtype == sample.dtype == numpy.int32
    assert points.tolist() == [[2.0, 0.0, 3.5], [3.0, -2.0, 4.0], [numpy.float32(0.3)] * 3] and points.dtype == numpy.float32
    offsets, sample, points = nref.select_ray_samples(origins, dirs, z_vals, weights, 0.25)
    assert offsets.tolist() == [0, 1, 2] and sample.tolist() == [1, 5]
    offsets, sample, points = nref.select_ray_samples(origins[:0], dirs[:0], z_vals[:0], weights[:0])
    assert offsets.tolist() == [0] and sample.shape == (0,) and points.shape == (0, 3)


def test_inverse_input_map_returns_to_q():
    """The restated inverse of the input map composed with the forward map of tests/field_reference.py returns Q.  With u = 2^-53
    the relative error of one fp64 operation and t = Q_z - 1 in [-2, 0):
      P_z = fl(2 near / fl(t)) carries (1 + e1)(1 + e2); the forward quotient fl(2 near / P_z) a third, so it is t (1 + d) with
      |d| <= 3 u to first order, and Q_z' = fl(1 + .) adds u |Q_z'|:  |Q_z' - Q_z| <= 3 u |t| + u |Q_z| <= 7 u for |Q_z| <= 1.
      P_x = fl(fl(Q_x P_z) / cx) and Q_x' = fl(fl(cx P_x) / P_z) are four operations on Q_x, and the one P_z divides out exactly:
      |Q_x' - Q_x| <= 4 u |Q_x| to first order; likewise y.
    Held to 8 u and 5 u |Q|: one u each for the second-order terms (at most 6 u^2 and 6 u^2 |Q|)."""
    ndc = field_reference.fern_cameras()[2]
    rng = numpy.random.default_rng(3)
    Q = rng.uniform(-1.0, 1.0, (2000, 3)).astype(numpy.float32)
    Q[:, 2] = rng.uniform(-1.0, 0.999, 2000).astype(numpy.float32)
    Q[0, 2], Q[1, 2] = -1.0, numpy.float32(0.999)
    worst_z = worst_xy = 0.0
    for row in Q:
        q = [float(v) for v in row]
        P, usable = nref.inverse_input_point(q, ndc)
        assert usable and P[2] <= -ndc[2]
        back, in_front, _ = field_reference.input_point(P, ndc)
        assert in_front
        worst_z = max(worst_z, abs(back[2] - q[2]) / U)
        for a in (0, 1):
            assert abs(back[a] - q[a]) <= 5 * U * abs(q[a]), (q, back)
            worst_xy = max(worst_xy, abs(back[a] - q[a]) / (U * abs(q[a])) if q[a] else 0.0)
        assert abs(back[2] - q[2]) <= 8 * U, (q, back)
    print(f'inverse input map: worst |Q_z\' - Q_z| = {worst_z:.2f} u [8 u], worst |Q_xy\' - Q_xy| = {worst_xy:.2f} u |Q| [5 u |Q|]')
    # at and past the far plane, and for a NaN, the sample is not usable
    for z in (1.0, 1.5, math.nan):
        assert not nref.inverse_input_point([0.1, 0.2, z], ndc)[1]
    assert not nref.inverse_input_point([0.1, 0.2, -1.5], ndc)[1]             # nearer than the near plane


def test_a_planar_slab_gives_the_slabs_normal():
    origins, dirs, z_vals, weights, points, inside = slab_case()
    offsets, sample, selected = nref.select_ray_samples(origins, dirs, z_vals, weights)
    assert selected.tobytes() == points.reshape(-1, 3)[sample].tobytes()       # the points the density was evaluated at
    enters = inside.any(axis=1)
    assert 20 <= int((~enters).sum()) <= 40 and not weights[~enters].any()
    normal, strength = nref.composite_normals(selected, slab_gradient(selected), offsets, sample, weights)
    want = slab_normal()
    hit = numpy.diff(offsets) > 0
    assert numpy.array_equal(hit, enters) or (hit <= enters).all()            # (a weight may underflow to 0, never the reverse)
    assert int(hit.sum()) >= 80
    assert numpy.abs(normal[hit].astype(numpy.float64) - want).max() <= 2.0 ** -24           # half a float32 ulp below 1
    sums = numpy.array([sum(float(w) for w in weights[r] if w > 0) for r in range(SLAB_RAYS)])
    assert numpy.abs(strength[hit] - sums[hit]).max() <= 2.0 ** -23 * sums[hit].max()
    assert not normal[~hit].any() and not strength[~hit].any()


def test_a_fronto_parallel_plane_gives_exactly_the_optical_axis():
    depth, cameras = fronto_parallel_case()
    assert numpy.array_equal(cameras[0, :9].reshape(3, 3), [[0.0625, 0.0, -0.5], [0.0, 0.0625, -0.25], [0.0, 0.0, 1.0]])
    for edge_threshold in (None, 0.05):
        normals = nref.depth_normals(depth, cameras, None, edge_threshold)
        assert normals.shape == (1, 9, 12, 3)
        assert numpy.array_equal(normals.reshape(-1, 3), numpy.tile(numpy.float32([0.0, 0.0, -1.0]), (108, 1)))      # towards the camera
    # a hole removes its own normal; its neighbours fall back to one-sided differences and keep theirs
    holed = depth.copy()
    holed[0, 4, 5] = numpy.nan
    normals = nref.depth_normals(holed, cameras)
    assert not normals[0, 4, 5].any() and numpy.array_equal(normals[0, 4, 4], [0.0, 0.0, -1.0])
    # a single pixel, a row and a column have no second tangent
    for shape in ((1, 1, 1), (1, 1, 5), (1, 5, 1)):
        assert not nref.depth_normals(numpy.full(shape, 2.0, numpy.float32), cameras).any()
    # a step beyond the edge threshold is not differenced across: the pixels beside it keep the axis
    stepped = depth.copy()
    stepped[0, :, 6:] = 5.0
    across = nref.depth_normals(stepped, cameras)
    kept = nref.depth_normals(stepped, cameras, None, 0.05)
    assert abs(across[0, 4, 5, 0]) > 0.5 and numpy.array_equal(kept[0, 4, 5], [0.0, 0.0, -1.0]) and numpy.array_equal(kept[0, 4, 6], [0.0, 0.0, -1.0])


def test_the_picture_of_a_normal():
    got = nref.normals_to_u8(numpy.float32([[0, 0, 0], [1, -1, 0.5], [2.0, -2.0, 0.25], [numpy.nan, 0.5, -0.5], [0.5, numpy.inf, 0.0]]))
    # (a NaN component spoils the whole row, an infinite one the other two: 0 . NaN and 0 . inf are NaN in the sums of R^T n)
    assert got.tolist() == [[128, 128, 128], [255, 0, 191], [255, 0, 159], [0, 0, 0], [0, 255, 0]]
    # a surface facing a camera that looks down -z comes out blue: the camera's +z axis, in the scene frame, is column 2 of R
    turned = numpy.array([[0.0, 0.0, 1.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])
    assert nref.normals_to_u8(numpy.float32([[0, 0, 1]])).tolist() == [[128, 128, 255]]
    assert nref.normals_to_u8(numpy.float32([turned[:, 2]]), turned).tolist() == [[128, 128, 255]]
    normals, rotation = picture_case()
    picture = nref.normals_to_u8(normals, rotation)
    assert picture.shape == (500, 3) and picture.dtype == numpy.uint8 and picture[0].tolist() == [128, 128, 128] and not picture[6].any()


# ------------------------------------------------------------------------------------------------------------------ the native program
def compile_smoke(out_dir):
    exe = os.path.join(out_dir, 'normals_abi_smoke')
    lib_dir = os.path.dirname(_lib.LIB_PATH)
    cmd = [build.HIPCC, '--offload-arch=gfx950', '-O1', '-std=c++17', f'-I{os.path.join(REPO, "include")}', f'-I{build.CSRC}',
           os.path.join(REPO, 'tests', 'native', 'normals_abi_smoke.cpp'), '-o', exe, f'-L{lib_dir}', '-lsimplenerf_hip',
           f'-Wl,-rpath,{lib_dir}']
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


@pytest.mark.skipif(not HAS_HIPCC, reason='hipcc not available')
def test_normals_abi_program_compiles_and_links(tmp_path):
    """CPU-side half of the native smoke: the new header is valid C++ for an outside consumer and the five symbols link."""
    build.build_library()
    assert os.path.exists(compile_smoke(str(tmp_path)))


NATIVE_RAYS, NATIVE_SAMPLES, NATIVE_MIN_WEIGHT, NATIVE_FRAMES, NATIVE_EDGE = 257, 65, 0.25, (3, 17, 33), 0.05


@functools.lru_cache(maxsize=None)
def native_fixture() -> bytes:
    """What tests/native/normals_abi_smoke.cpp reads, little-endian: int32 rays, samples, selected M, views, height, width |
    float64 min_weight, cx, cy, near, edge_threshold, rotation (9) | float32 origins (R,3), dirs (R,3), z_vals (R,S), weights (R,S)
    | int32 offsets (R+1), sample (M) | float32 points (M,3), grad (M,3), normal (R,3), strength (R): the restatement's, with the NDC
    pull-back | float64 cameras (V,42) | float32 depth (V,h,w) | uint8 mask (V,h,w) | float32 depth normals (V,h,w,3) | uint8 the
    picture of `normal` (R,3)."""
    origins, dirs, z_vals, weights = selection_case(NATIVE_RAYS, NATIVE_SAMPLES)
    origins, dirs = (0.1 * origins).astype(numpy.float32), (0.2 * dirs).astype(numpy.float32)      # keep the NDC points near the cube
    z_vals = (z_vals / 6.0).astype(numpy.float32)
    ndc = field_reference.fern_cameras()[2]
    offsets, sample, points = nref.select_ray_samples(origins, dirs, z_vals, weights, NATIVE_MIN_WEIGHT)
    rng = numpy.random.default_rng(77)
    grad = rng.standard_normal(points.shape).astype(numpy.float32)
    grad[::13] = 0.0
    normal, strength = nref.composite_normals(points, grad, offsets, sample, weights, ndc)
    assert int((strength > 0).sum()) > NATIVE_RAYS // 2 and int((strength == 0).sum()) > NATIVE_RAYS // 6
    depth, mask, cameras, _, _ = depth_case(*NATIVE_FRAMES)
    depth_normals = nref.depth_normals(depth, cameras, mask, NATIVE_EDGE)
    rotation = picture_case()[1]
    image = nref.normals_to_u8(normal, rotation)
    little = lambda array, dtype: numpy.ascontiguousarray(array).astype(dtype).tobytes()
    parts = [struct.pack('<6i14d', NATIVE_RAYS, NATIVE_SAMPLES, len(sample), *NATIVE_FRAMES, NATIVE_MIN_WEIGHT, *ndc, NATIVE_EDGE,
                         *rotation.reshape(-1).tolist()),
             little(origins, '<f4'), little(dirs, '<f4'), little(z_vals, '<f4'), little(weights, '<f4'), little(offsets, '<i4'),
             little(sample, '<i4'), little(points, '<f4'), little(grad, '<f4'), little(normal, '<f4'), little(strength, '<f4'),
             little(cameras, '<f8'), little(depth, '<f4'), little(mask, 'u1'), little(depth_normals, '<f4'), little(image, 'u1')]
    return b''.join(parts)


def test_native_fixture_layout():
    data = native_fixture()
    rays, samples, count, views, height, width = numpy.frombuffer(data[:24], '<i4').tolist()
    assert (rays, samples, views, height, width) == (NATIVE_RAYS, NATIVE_SAMPLES) + NATIVE_FRAMES and 0 < count < rays * samples
    pixels = views * height * width
    assert len(data) == 24 + 14 * 8 + 4 * (6 * rays + 2 * rays * samples) + 4 * (rays + 1 + count) + 4 * (6 * count + 4 * rays) \
        + 8 * 42 * views + 4 * pixels + pixels + 12 * pixels + 3 * rays
