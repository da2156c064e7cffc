"""The field export restated in plain Python / numpy float64, node by node and point by point, in the words of
simplenerf_amd/csrc/simplenerf_field.h: what tests/test_field_host.py pins on the CPU and tests/test_gpu_field.py holds the device
to.  The lookup follows tests/mesh_reference.py's ``look_up`` (the same sentences of simplenerf_mesh.h, without the depth read), the
cameras are the (V,42) table of simplenerf_fuse.h, the scene and the extraction are mesh_reference's.

Nothing here is vectorised over nodes or points on purpose: every step is one sentence of a rule, every sum and product is one Python
float operation in the order the header gives (Python floats are IEEE doubles; nothing is fused)."""
import functools
import math
import struct

import numpy

from . import mesh_reference

NO_VIEW = 255
E_INV, E, K = 9, 21, 33            # offsets of inv(E)[:3], E[:3] and K in a view's row of the camera table
_divide = mesh_reference._divide


# ---------------------------------------------------------------------------------------------------------------- the input map
def input_point(P, ndc):
    """THE INPUT MAP -> (Q: three floats, in front: bool, margin: the distance of the in-front decision from its threshold)."""
    if ndc is None:
        return [P[0], P[1], P[2]], True, math.inf
    cx, cy, near = (float(v) for v in ndc)
    margin = abs(P[2] + near) if P[2] == P[2] else math.inf
    if not P[2] <= -near:
        return [0.0, 0.0, 0.0], False, margin
    return [_divide(cx * P[0], P[2]), _divide(cy * P[1], P[2]), 1.0 + _divide(2.0 * near, P[2])], True, margin


def sees(P, table, u, height, width):
    """THE LOOKUP of ``P`` in view ``u`` up to the depth read -> (seen: bool, c_z, margin: how far the nearest of its decisions -- c_z
    against 0, a tie of rint, which the frame's edges are too -- lies from turning over)."""
    row = table[u]
    c = [((float(row[E + 4 * a]) * P[0] + float(row[E + 4 * a + 1]) * P[1]) + float(row[E + 4 * a + 2]) * P[2]) + float(row[E + 4 * a + 3])
         for a in range(3)]
    if c[2] != c[2]:
        return False, c[2], math.inf
    if not c[2] > 0:
        return False, c[2], abs(c[2])
    q = [(float(row[K + 3 * a]) * c[0] + float(row[K + 3 * a + 1]) * c[1]) + float(row[K + 3 * a + 2]) * c[2] for a in range(3)]
    px, py = _divide(q[0], q[2]), _divide(q[1], q[2])
    ix, iy = float(numpy.rint(px)), float(numpy.rint(py))              # ties to even
    margin = abs(c[2])
    if math.isfinite(px) and math.isfinite(py):
        margin = min(margin, abs(abs(px - math.floor(px)) - 0.5), abs(abs(py - math.floor(py)) - 0.5))
    return bool(0 <= ix < width and 0 <= iy < height), c[2], margin   # (a NaN fails every comparison)


# ---------------------------------------------------------------------------------------------------------------- the three calls
def grid_points(lo, voxel_size, extents, table, resolution, ndc=None, first_node=0, count=None, margins=None):
    """-> (mlp_points float32 (count, 3), weight uint8 (count)).  ``margins``: a list that receives each node's smallest margin."""
    nx, ny, nz = extents
    height, width = resolution
    table = numpy.asarray(table, dtype=numpy.float64).reshape(-1, 42)
    views = len(table) if height * width > 0 else 0
    count = nx * ny * nz - first_node if count is None else count
    points = numpy.zeros((count, 3), dtype=numpy.float32)
    weight = numpy.zeros((count,), dtype=numpy.uint8)
    for at in range(count):
        n = first_node + at
        P = mesh_reference.node_position(lo, voxel_size, (n % nx, n // nx % ny, n // (nx * ny)))
        Q, in_front, margin = input_point(P, ndc)
        seen = 0
        if in_front:
            for u in range(views):
                yes, _, m = sees(P, table, u, height, width)
                margin = min(margin, m)
                seen += yes
        points[at] = Q
        weight[at] = seen
        if margins is not None:
            margins.append(margin)
    return points, weight


def point_views(points, table, resolution, ndc=None, margins=None):
    """-> (mlp_points float32 (count, 3), view_dirs float32 (count, 3), view uint8 (count)).  ``margins``: a list that receives, per
    point, the smaller of its decisions' margins and of the gap between the two smallest depths of the views that see it."""
    points = numpy.asarray(points, dtype=numpy.float32)
    height, width = resolution
    table = numpy.asarray(table, dtype=numpy.float64).reshape(-1, 42)
    views = len(table) if height * width > 0 else 0
    mlp_points = numpy.zeros((len(points), 3), dtype=numpy.float32)
    view_dirs = numpy.zeros((len(points), 3), dtype=numpy.float32)
    view = numpy.zeros((len(points),), dtype=numpy.uint8)
    for at, point in enumerate(points):
        P = [float(point[0]), float(point[1]), float(point[2])]
        Q, in_front, margin = input_point(P, ndc)
        depths = []
        if in_front:
            for u in range(views):
                yes, c_z, m = sees(P, table, u, height, width)
                margin = min(margin, m)
                if yes:
                    depths.append((c_z, u))
        chosen = min(depths)[1] if depths else None                    # the smallest c_z, the lowest index among equal ones
        if len(depths) > 1:
            ordered = sorted(depths)
            margin = min(margin, ordered[1][0] - ordered[0][0])
        row = table[0 if chosen is None else chosen]
        v = [P[a] - float(row[E_INV + 4 * a + 3]) for a in range(3)]
        with numpy.errstate(invalid='ignore', over='ignore'):
            n = float(numpy.sqrt(numpy.float64((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])))
        mlp_points[at] = Q
        with numpy.errstate(invalid='ignore', over='ignore'):
            view_dirs[at] = [0.0, 0.0, 0.0] if n == 0 else [_divide(v[a], n) for a in range(3)]
        view[at] = NO_VIEW if chosen is None else chosen
        if margins is not None:
            margins.append(margin)
    return mlp_points, view_dirs, view


def values(sigma, weight, level):
    """-> tsdf float32, shaped like ``sigma``."""
    sigma = numpy.asarray(sigma, dtype=numpy.float32)
    weight = numpy.asarray(weight, dtype=numpy.uint8)
    level = float(level)
    tsdf = numpy.ones(sigma.shape, dtype=numpy.float32)
    flat = tsdf.reshape(-1)
    for at, (s, w) in enumerate(zip(sigma.reshape(-1).tolist(), weight.reshape(-1).tolist())):
        if w == 0 or s != s:
            continue
        flat[at] = numpy.float32(min(1.0, max(-1.0, _divide(level - s, level))))
    return tsdf


# ---------------------------------------------------------------------------------------------------------------- the scenes
SMALL_EXTENTS, SMALL_VOXEL = (13, 12, 11), 0.25                          # 1716 nodes over the sphere scene: not a multiple of any tile
SMALL_LO = mesh_reference.GRID_LO
SCENE_RESOLUTION = (mesh_reference.SCENE_SIZE, mesh_reference.SCENE_SIZE)
SPHERE_LEVEL = 20.0                                                     # 40 max(0, 1 - |p| / 1.2) = 20 on the sphere of radius 0.6


@functools.lru_cache(maxsize=None)
def scene_table():
    """The (6, 42) camera table of mesh_reference.scene(); read-only."""
    from simplenerf_amd import geometry
    s = mesh_reference.scene()
    table = geometry.fuse_cameras(s['extrinsics'], s['intrinsics'])
    table.setflags(write=False)
    return table


@functools.lru_cache(maxsize=None)
def scene_grid_points(extents=SMALL_EXTENTS, voxel_size=SMALL_VOXEL, lo=SMALL_LO):
    """The restated points and weights of a grid over the sphere scene: (points, weight, margins); read-only."""
    margins = []
    points, weight = grid_points(lo, voxel_size, extents, scene_table(), SCENE_RESOLUTION, None, 0, None, margins)
    points.setflags(write=False)
    weight.setflags(write=False)
    return points, weight, tuple(margins)


def sphere_density(points):
    """sigma = 40 max(0, 1 - |p| / 1.2) in float32 steps (numpy), the field of the analytic test: (n, 3) -> (n,)."""
    points = numpy.asarray(points, dtype=numpy.float32)
    radius = numpy.sqrt((points * points).sum(axis=1, dtype=numpy.float32))
    return (numpy.float32(40.0) * numpy.maximum(numpy.float32(0.0), numpy.float32(1.0) - radius / numpy.float32(1.2))).astype(numpy.float32)


def fern_cameras(count=3, resolution=(48, 64)):
    """``count`` forward-facing cameras of the fern scene at a small frame size -> (camera dicts, (V,42) table, (cx, cy, near))."""
    from simplenerf_amd import geometry, synth
    cameras = [synth.camera('fern', i, resolution=resolution) for i in range(count)]
    matrices = [geometry.camera_matrices(camera) for camera in cameras]
    table = geometry.fuse_cameras(numpy.stack([m[0] for m in matrices]), numpy.stack([m[1] for m in matrices]))
    return cameras, table, geometry.ndc_parameters(cameras[0])


# ---------------------------------------------------------------------------------------------------------------- the native fixture
NATIVE_MLP = dict(depth=4, width=128, views_width=64)
NATIVE_SEED, NATIVE_GAIN, NATIVE_SHIFT = 11, 150.0, 4.0


def native_mlp():
    """(MLP config, parameters in C-ABI order as float32 arrays) of the seeded 4 x 128 / 64 MLP the native program evaluates."""
    from simplenerf_amd import synth

    from . import util
    cfg = synth.mlp_config(64, **NATIVE_MLP)
    state = synth.synth_state_dict(util.mlp_param_shapes(cfg), NATIVE_SEED, NATIVE_GAIN, NATIVE_SHIFT)
    return cfg, synth.abi_param_list(state)


def native_fixture(level=1.0, counts=(-1, -1)) -> bytes:
    """What tests/native/field_abi_smoke.cpp reads, little-endian, in this order:
    int32 views, h, w, nx, ny, nz, params | float64 voxel_size, lo (3), level | int64 Nv, Nt (-1: not known) | float64 cameras
    (views, 42) | float32 points (nodes, 3) | uint8 weight (nodes) | per parameter: int64 its number of floats, float32 its values
    -- the sphere scene's cameras, the restated points and weights of the small grid over it, and the seeded MLP."""
    points, weight, _ = scene_grid_points()
    params = native_mlp()[1]
    little = lambda array, dtype: numpy.ascontiguousarray(array).astype(dtype).tobytes()
    parts = [struct.pack('<7i5d2q', len(scene_table()), *SCENE_RESOLUTION, *SMALL_EXTENTS, len(params), SMALL_VOXEL, *SMALL_LO, float(level),
                         int(counts[0]), int(counts[1])),
             little(scene_table(), '<f8'), little(points, '<f4'), little(weight, 'u1')]
    for value in params:
        parts += [struct.pack('<q', value.size), little(value, '<f4')]
    return b''.join(parts)
