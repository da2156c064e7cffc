"""The geometry a model has learnt, as something a 3-D viewer opens: the depth maps of several views fused into one coloured point
cloud, or into a triangle mesh, and written as a binary PLY file.

A depth map alone puts a point behind every pixel, floaters included.  ``fuse_depth_maps`` keeps a pixel's point only where other
views confirm it: the point is projected into every other view and compared with the depth that view holds at the pixel it lands on
(nearest pixel, one-way check, relative threshold) -- the consistency filter of multi-view stereo toolkits, on the device
(csrc/fuse.hip; csrc/simplenerf_fuse.h states the rule, tests/fuse_reference.py restates it in numpy).  ``voxel_thin`` then leaves
one averaged point per occupied voxel.  Conventions are those of ``qa.visibility_mask`` and ``qa.forward_warp``: integer pixel
coordinates (x = column, y = row), z-depths in the extrinsics' units, extrinsics 4x4 world-to-camera and intrinsics 3x3 (numpy or
tensor), composed on the host in float64; fp64 device arithmetic without atomics, so the same input gives the same bits.

A surface comes from the same depth maps in three steps (csrc/mesh.hip; csrc/simplenerf_mesh.h states the rules, tests/mesh_reference.py
restates them): ``tsdf_volume`` averages truncated signed distances into a regular grid, ``extract_mesh`` runs marching tetrahedra
over it (six Kuhn tetrahedra a cell: no ambiguous case, watertight wherever the volume is observed), ``colour_points`` colours the
vertices from the frames; ``save_ply_mesh`` writes the indexed file.

The density field is meshed without a render (csrc/field.hip; csrc/simplenerf_field.h states the rules, tests/field_reference.py
restates them): ``density_volume`` maps the grid's nodes into the space the model's MLP reads (the NDC warp for LLFF models),
counts the views that see each, asks the field for its densities there and turns them into the signed volume of a density level;
``extract_mesh`` meshes it as above; ``colour_vertices`` asks the field for the colour of every vertex, seen from the nearest
camera that sees it.

``field_normals`` gives the density mesh's vertices the unit outward normals of the field's own gradient (``model.query_gradient``;
csrc/simplenerf_gradient.h), which ``save_ply_mesh(..., normals=)`` and ``save_ply(..., normals=)`` write; the depth mesh's
vertices and the fused cloud's points take the same normals.

A rendered frame has two normal maps (csrc/normals.hip; csrc/simplenerf_normals.h states the rules, tests/normals_reference.py
restates them): ``ray_normals`` composites the field's normals along every ray with the render's own weights, over the samples that
carry weight; ``depth_normals`` differences the points of neighbouring pixels of the depth map; ``normals_to_u8`` makes either a
picture.  Where the two disagree the geometry is not a surface yet.

Out of scope: marching cubes, Poisson reconstruction, bilinear depth lookups, view-angle or distance
weighting, sparse or hashed volumes, dropping zero-area triangles, welding coincident vertices, two-way reprojection checks,
sharding over ranks, ASCII PLY; for the density mesh also a density-only forward that skips the feature and views layers,
empty-space culling, default bounds, the opacity of a voxel step as the level-set quantity, and gradients in the 16-bit modes, for
layered MLP shapes and of the colour; for the normal maps also compositing from the render's own kept activations instead of a
second forward, normals of the coarse or augmentation levels, normal losses or supervision, normals in the view sweep and the
videos, and smoothing or bilateral filtering of depth normals.
"""
from __future__ import annotations

import os
from typing import Optional

import numpy
import torch

from . import ops
from .qa import _matrices

Tensor = torch.Tensor
PLY_FACE = numpy.dtype([('count', 'u1'), ('a', '<i4'), ('b', '<i4'), ('c', '<i4')])     # 13 bytes
PLY_VERTEX = numpy.dtype([('x', '<f4'), ('y', '<f4'), ('z', '<f4'), ('red', 'u1'), ('green', 'u1'), ('blue', 'u1')])     # 15 bytes


def fuse_cameras(extrinsics, intrinsics) -> numpy.ndarray:
    """The (V,42) float64 table ``ops.fuse_depth_maps`` takes, inverted on the host: per view inv(K) | rows 0..2 of inv(E) | rows
    0..2 of E | K, row-major.  ``extrinsics`` (V,4,4) world-to-camera, ``intrinsics`` (V,3,3)."""
    views = len(extrinsics)
    e = _matrices(extrinsics, 'extrinsics', (views, 4, 4))
    k = _matrices(intrinsics, 'intrinsics', (views, 3, 3))
    table = numpy.empty((views, ops.FUSE_CAMERA), dtype=numpy.float64)
    for v in range(views):
        table[v, 0:9] = numpy.linalg.inv(k[v]).reshape(-1)
        table[v, 9:21] = numpy.linalg.inv(e[v])[:3].reshape(-1)
        table[v, 21:33] = e[v, :3].reshape(-1)
        table[v, 33:42] = k[v].reshape(-1)
    return table


def fuse_depth_maps(depth: Tensor, image: Tensor, extrinsics, intrinsics, depth_error_threshold: float = 0.02, min_views: int = 1,
                    mask: Optional[Tensor] = None):
    """-> (points float32 (N,3), colours uint8 (N,3), views uint8 (N)) on the device: the fused cloud of the float32 (V,h,w) ``depth``
    maps and uint8 (V,h,w,3) ``image`` frames on the GPU.  A pixel is valid where its depth is finite and positive and ``mask`` (bool
    or uint8 (V,h,w) on the GPU, optional) is set; its point P = inv(E)[:3] [d inv(K) (x, y, 1); 1] is kept when at least
    ``min_views`` (0..V-1) of the other views agree: P lies in front of the view, projects (rounded to the nearest pixel, ties to
    even) inside its frame onto a valid pixel of depth d_u, and |z - d_u| <= ``depth_error_threshold`` x d_u for P's depth z in that
    view.  Points come in ascending (view, row, column) order with the pixel's colour; ``views`` is the number of agreeing views."""
    if not isinstance(depth, torch.Tensor) or depth.dim() != 3:
        raise RuntimeError(f'depth: expected a float32 tensor of shape (views, h, w) on the GPU, got '
                           f'{tuple(depth.shape) if isinstance(depth, torch.Tensor) else type(depth).__name__}')
    views = int(depth.shape[0])
    cameras = fuse_cameras(_matrices(extrinsics, 'extrinsics', (views, 4, 4)), _matrices(intrinsics, 'intrinsics', (views, 3, 3)))
    return ops.fuse_depth_maps(depth, image, torch.from_numpy(cameras).to(depth.device), depth_error_threshold, min_views, mask)


def voxel_thin(points: Tensor, colours: Tensor, voxel_size: float):
    """-> (points float32 (M,3), colours uint8 (M,3), counts int32 (M)) on the device: one record per voxel of side ``voxel_size``
    (the grid starts at the per-axis minimum of ``points``) that holds a point -- the mean position, the rounded mean colour, the
    number of points -- in ascending voxel order (z, then y, then x).  Raises when a bound of the cloud is not finite or the grid
    would have more than 2^31 - 1 voxels."""
    return ops.voxel_thin(points, colours, voxel_size)


def camera_matrices(camera: dict):
    """-> (extrinsic (4,4), intrinsic (3,3)) float64 of a camera dict as ``harness.frame_batch`` takes it.  Its ``pose`` is the
    processed camera-to-world matrix with the camera looking down -z, y up (the ray generator flips y and z of inv(K) (x, y, 1));
    the extrinsic here is world-to-camera with the camera looking down +z, y down, so that
    inv(E)[:3] [t inv(K) (x, y, 1); 1] = rays_o + t rays_d and a rendered depth is the z-depth the fuse expects."""
    pose = numpy.asarray(camera['pose'], dtype=numpy.float64).reshape(4, 4)
    intrinsic = numpy.asarray(camera['intrinsic'], dtype=numpy.float64).reshape(3, 3)
    camera_to_world = numpy.matmul(pose, numpy.diag([1.0, -1.0, -1.0, 1.0]))
    return numpy.linalg.inv(camera_to_world), intrinsic.copy()


PLY_VERTEX_NORMAL = numpy.dtype([('x', '<f4'), ('y', '<f4'), ('z', '<f4'), ('nx', '<f4'), ('ny', '<f4'), ('nz', '<f4'),
                                 ('red', 'u1'), ('green', 'u1'), ('blue', 'u1')])     # 27 bytes


def ply_bytes(points, colours, normals=None) -> bytes:
    """A binary little-endian PLY file of N vertices: float x, y, z and uchar red, green, blue, 15 bytes a record.  ``points`` (N,3)
    float32 and ``colours`` (N,3) uint8, tensors (copied to the host) or numpy; N = 0 is a valid file.  With ``normals`` (N,3)
    float32 the vertex element is ``x y z nx ny nz red green blue``, 27 bytes a record (oriented normals, as a surface
    reconstruction reads them); without, the file is what it was before normals existed.  ``ply_mesh_bytes`` writes its vertex
    element through this function."""
    if isinstance(points, torch.Tensor):
        points = points.detach().cpu().numpy()
    if isinstance(colours, torch.Tensor):
        colours = colours.detach().cpu().numpy()
    points, colours = numpy.asarray(points), numpy.asarray(colours)
    if points.dtype != numpy.float32 or points.ndim != 2 or points.shape[1] != 3:
        raise RuntimeError(f'points: expected float32 (N, 3), got {points.dtype} {points.shape}')
    if colours.dtype != numpy.uint8 or colours.shape != points.shape:
        raise RuntimeError(f'colours: expected uint8 {points.shape}, got {colours.dtype} {colours.shape}')
    if normals is not None:
        if isinstance(normals, torch.Tensor):
            normals = normals.detach().cpu().numpy()
        normals = numpy.asarray(normals)
        if normals.dtype != numpy.float32 or normals.shape != points.shape:
            raise RuntimeError(f'normals: expected float32 {points.shape}, got {normals.dtype} {normals.shape}')
    records = numpy.empty((points.shape[0],), dtype=PLY_VERTEX if normals is None else PLY_VERTEX_NORMAL)
    for a, name in enumerate(('x', 'y', 'z')):
        records[name] = points[:, a]
    for a, name in enumerate(('red', 'green', 'blue')):
        records[name] = colours[:, a]
    if normals is not None:
        for a, name in enumerate(('nx', 'ny', 'nz')):
            records[name] = normals[:, a]
    header = ('ply\nformat binary_little_endian 1.0\n' + f'element vertex {points.shape[0]}\n'
              + 'property float x\nproperty float y\nproperty float z\n'
              + ('' if normals is None else 'property float nx\nproperty float ny\nproperty float nz\n')
              + 'property uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n')
    return header.encode('ascii') + records.tobytes()


def save_ply(path, points, colours, normals=None) -> None:
    """``ply_bytes`` written to ``path``.  A file that exists is left alone, as ``harness.save_video`` leaves it."""
    path = os.fspath(path)
    if os.path.exists(path):
        return
    data = ply_bytes(points, colours, normals)
    os.makedirs(os.path.dirname(path) or '.', exist_ok=True)
    with open(path, 'wb') as f:
        f.write(data)


# ---------------------------------------------------------------------------------------------------------------- the mesh
def _views_of(depth, extrinsics, intrinsics):
    if not isinstance(depth, torch.Tensor) or depth.dim() != 3:
        raise RuntimeError(f'depth: expected a float32 tensor of shape (views, h, w) on the GPU, got '
                           f'{tuple(depth.shape) if isinstance(depth, torch.Tensor) else type(depth).__name__}')
    views = int(depth.shape[0])
    cameras = fuse_cameras(_matrices(extrinsics, 'extrinsics', (views, 4, 4)), _matrices(intrinsics, 'intrinsics', (views, 3, 3)))
    return torch.from_numpy(cameras.reshape(views, ops.FUSE_CAMERA)).to(depth.device)


def tsdf_volume(depth: Tensor, extrinsics, intrinsics, lo, voxel_size: float, extents, truncation: float, mask: Optional[Tensor] = None):
    """-> (tsdf float32 (nz,ny,nx), weight uint8 (nz,ny,nx)) on the device: the float32 (V,h,w) ``depth`` maps on the GPU fused into
    the grid of ``extents`` = (nx,ny,nz) nodes whose node (i,j,k) sits at ``lo`` + ``voxel_size`` (i,j,k).  A view contributes to a
    node that lies in front of it and projects (nearest pixel, ties to even) inside its frame onto a valid pixel (finite positive
    depth d, ``mask`` set) no more than ``truncation`` in front of the node: min(1, (d - z) / truncation) for the node's depth z in
    that view.  ``tsdf`` is the mean over the contributing views (1 where there is none), ``weight`` their number."""
    return ops.tsdf_integrate(depth, _views_of(depth, extrinsics, intrinsics), lo, voxel_size, extents, truncation, mask)


def extract_mesh(tsdf: Tensor, weight: Tensor, lo, voxel_size: float, min_weight: int = 1):
    """-> (vertices float32 (Nv,3), triangles int32 (Nt,3)) on the device: the surface tsdf = 0 by marching tetrahedra over the cells
    of the volume whose eight nodes all have ``weight`` >= ``min_weight``.  A vertex lies on a grid edge whose nodes differ in sign
    (a node is negative where tsdf < 0), interpolated linearly; triangles are wound so that their normals look from the negative side
    to the positive one, i.e. out of the surface and towards the cameras.  Zero-area triangles (a surface through a node) are kept."""
    return ops.mesh_extract(tsdf, weight, lo, voxel_size, min_weight)


def colour_points(points: Tensor, depth: Tensor, image: Tensor, extrinsics, intrinsics, colour_tolerance: float,
                  mask: Optional[Tensor] = None):
    """-> (colours uint8 (N,3), views uint8 (N)) on the device: every float32 (N,3) point coloured with the rounded mean of the
    uint8 (V,h,w,3) ``image`` pixels it projects to in the views whose valid depth there is within ``colour_tolerance`` (scene units)
    of the point's own depth in that view; ``views`` counts them, and the colour is (0,0,0) where it is 0."""
    return ops.colour_points(points, depth, image, _views_of(depth, extrinsics, intrinsics), colour_tolerance, mask)


# ---------------------------------------------------------------------------------------------------------------- the field
def ndc_parameters(camera: dict):
    """-> (cx, cy, near) float64: the parameters of the NDC warp of a camera dict as ``harness.frame_batch`` takes it, evaluated as the
    ray generator evaluates them in fp32: cx = -1 / (W / (2 fx)), cy = -1 / (H / (2 fy)); near is the camera's near plane."""
    h, w = (int(v) for v in camera['resolution'])
    intrinsic = numpy.asarray(camera['intrinsic'], dtype=numpy.float64).reshape(3, 3)
    cx = -1.0 / (float(w) / (2.0 * float(intrinsic[0, 0])))
    cy = -1.0 / (float(h) / (2.0 * float(intrinsic[1, 1])))
    return cx, cy, float(camera['near'])


def _field_cameras(extrinsics, intrinsics, device):
    views = len(extrinsics)
    cameras = fuse_cameras(_matrices(extrinsics, 'extrinsics', (views, 4, 4)), _matrices(intrinsics, 'intrinsics', (views, 3, 3)))
    return torch.from_numpy(cameras.reshape(views, ops.FUSE_CAMERA)).to(device)


def density_volume(query, lo, voxel_size: float, extents, extrinsics, intrinsics, resolution, level: float, ndc=None,
                   point_block: int = 1 << 20, device=None):
    """-> (sigma float32, tsdf float32, weight uint8), each (nz,ny,nx) on the device: the density field ``query`` sampled at the
    nodes of the grid of ``extents`` = (nx,ny,nz) whose node (i,j,k) sits at ``lo`` + ``voxel_size`` (i,j,k), in the scene frame of
    the (V,4,4) world-to-camera ``extrinsics``.  ``query`` is any callable from float32 (n,3) device points, in the space the model's
    MLP reads, to float32 (n,) densities; ``ndc`` = (cx, cy, near) (``ndc_parameters``) maps the nodes there for a model of NDC
    rays, None leaves them as they are.  ``weight`` counts the views that see a node (in front of the view, and projecting inside
    its (height, width) = ``resolution`` frame); ``tsdf`` = clamp((``level`` - sigma) / ``level``, -1, 1), and 1 where no view sees
    the node or the density is a NaN: the volume ``extract_mesh`` takes, whose surface is the level set sigma = ``level`` with
    normals out of the dense side.  The grid is walked in blocks of ``point_block`` nodes; nodes that no view sees are queried too.
    ``device`` defaults to the current GPU."""
    level = float(level)
    if not (level > 0.0 and numpy.isfinite(level)):
        raise RuntimeError(f'level: expected a finite number > 0, got {level}')
    if isinstance(point_block, bool) or int(point_block) != point_block or int(point_block) < 1:
        raise RuntimeError(f'point_block: expected an integer >= 1, got {point_block}')
    lo, voxel_size, extents = ops.mesh_grid(lo, voxel_size, extents)
    device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
    cameras = _field_cameras(extrinsics, intrinsics, device)
    nx, ny, nz = extents
    nodes = nx * ny * nz
    sigma = torch.empty((nodes,), dtype=torch.float32, device=device)
    weight = torch.empty((nodes,), dtype=torch.uint8, device=device)
    for first in range(0, nodes, int(point_block)):
        count = min(int(point_block), nodes - first)
        points, weight[first:first + count] = ops.field_grid_points(lo, voxel_size, extents, cameras, resolution, ndc, first, count)
        values = query(points)
        if not isinstance(values, torch.Tensor) or values.dtype != torch.float32 or tuple(values.shape) != (count,):
            raise RuntimeError(f'query: expected float32 densities of shape ({count},), got '
                               f'{(values.dtype, tuple(values.shape)) if isinstance(values, torch.Tensor) else type(values).__name__}')
        sigma[first:first + count] = values
    tsdf = ops.field_values(sigma, weight, level)
    return sigma.reshape(nz, ny, nx), tsdf.reshape(nz, ny, nx), weight.reshape(nz, ny, nx)


def colour_vertices(query, vertices: Tensor, extrinsics, intrinsics, resolution, ndc=None):
    """-> (colours uint8 (Nv,3), views uint8 (Nv)) on the device: the colour the field gives every float32 (Nv,3) scene-frame vertex,
    seen from the camera that sees it from the smallest depth; ``views`` is that camera's index, or ``ops.FIELD_NO_VIEW`` where none
    sees the vertex (camera 0's direction is used).  ``query`` is any callable from (float32 (n,3) points in the MLP's input space,
    float32 (n,3) unit view directions in the scene frame) to float32 (n,3) colours in [0, 1]; they are converted as
    ``ops.to_display`` converts a frame."""
    vertices = ops._typed(vertices, 'vertices', (torch.float32,))
    cameras = _field_cameras(extrinsics, intrinsics, vertices.device)
    points, view_dirs, views = ops.field_point_views(vertices, cameras, resolution, ndc)
    count = int(points.shape[0])
    if count == 0:
        return torch.empty((0, 3), dtype=torch.uint8, device=vertices.device), views
    rgb = query(points, view_dirs)
    if not isinstance(rgb, torch.Tensor) or rgb.dtype != torch.float32 or tuple(rgb.shape) != (count, 3):
        raise RuntimeError(f'query: expected float32 colours of shape ({count}, 3), got '
                           f'{(rgb.dtype, tuple(rgb.shape)) if isinstance(rgb, torch.Tensor) else type(rgb).__name__}')
    return ops.to_display(rgb)[0], views


def field_normals(query_gradient, vertices: Tensor, ndc=None) -> Tensor:
    """-> normals float32 (Nv,3) on the device: the unit outward normal of the density field at every float32 (Nv,3) scene-frame
    vertex, from the field's own gradient instead of the triangles (whose facets carry the pattern of the six tetrahedra).
    ``query_gradient`` is any callable from float32 (n,3) device points, in the space the model's MLP reads, to the float32 (n,3)
    gradient of the density there (``lambda p: model.query_gradient(p)['grad']``); ``ndc`` = (cx, cy, near) maps the vertices there
    for a model of NDC rays, as ``density_volume`` maps the nodes, and the gradient is pulled back through that map
    (``ops.field_normals``).  (0, 0, 0) where the gradient is zero or not finite, or the vertex is nearer than the near plane."""
    vertices = ops._typed(vertices, 'vertices', (torch.float32,))
    if vertices.dim() != 2 or vertices.shape[1] != 3:
        raise RuntimeError(f'vertices: expected shape (Nv, 3), got {tuple(vertices.shape)}')
    count = int(vertices.shape[0])
    if count == 0:
        return torch.empty((0, 3), dtype=torch.float32, device=vertices.device)
    points = vertices
    if ndc is not None:       # (the input map alone: one camera row that is never looked at, frames without pixels)
        cameras = torch.zeros((1, ops.FUSE_CAMERA), dtype=torch.float64, device=vertices.device)
        points = ops.field_point_views(vertices, cameras, (0, 0), ndc)[0]
    grad = query_gradient(points)
    if not isinstance(grad, torch.Tensor) or grad.dtype != torch.float32 or tuple(grad.shape) != (count, 3):
        raise RuntimeError(f'query_gradient: expected float32 gradients of shape ({count}, 3), got '
                           f'{(grad.dtype, tuple(grad.shape)) if isinstance(grad, torch.Tensor) else type(grad).__name__}')
    return ops.field_normals(vertices, grad, ndc)


# ---------------------------------------------------------------------------------------------------------------- normal maps
def ray_normals(query_gradient, rays_o: Tensor, rays_d: Tensor, z_vals: Tensor, weights: Tensor, ndc=None, min_weight: float = 0.0):
    """-> (normals float32 (R,3), strength float32 (R), selected M) : the field's own normals composited along the rays of a render
    with the render's weights.  The samples whose float32 (R,S) ``weights`` exceed ``min_weight`` are selected with the points the
    MLP saw, ``rays_o`` + ``rays_d`` x ``z_vals`` in float32 (``ops.select_ray_samples``; the density's ReLU leaves exact zero weights
    in empty space, and those samples cost no gradient); ``query_gradient`` -- any callable from float32 (n,3) device points, in the
    space the model's MLP reads, to the float32 (n,3) gradient of the density there, as ``field_normals`` takes it -- is asked at
    them once; and every ray sums weight x unit normal over its samples, in the scene frame (``ops.composite_normals``; ``ndc`` =
    (cx, cy, near) for a render of NDC rays, whose ``rays_o``, ``rays_d`` and ``z_vals`` are the NDC ones).  ``normals`` is that
    sum's direction and ``strength`` its length: at most the sum of the selected weights, less where the samples' normals disagree;
    both 0 for a ray without a usable sample."""
    offsets, sample, points = ops.select_ray_samples(rays_o, rays_d, z_vals, weights, min_weight)
    count = int(points.shape[0])
    if count > 0:
        grad = query_gradient(points)
        if not isinstance(grad, torch.Tensor) or grad.dtype != torch.float32 or tuple(grad.shape) != (count, 3):
            raise RuntimeError(f'query_gradient: expected float32 gradients of shape ({count}, 3), got '
                               f'{(grad.dtype, tuple(grad.shape)) if isinstance(grad, torch.Tensor) else type(grad).__name__}')
    else:
        grad = torch.empty((0, 3), dtype=torch.float32, device=points.device)
    normals, strength = ops.composite_normals(points, grad, offsets, sample, weights, ndc)
    return normals, strength, count


def depth_normals(depth: Tensor, extrinsics, intrinsics, mask: Optional[Tensor] = None, edge_threshold: Optional[float] = None) -> Tensor:
    """-> float32 (V,h,w,3) on the device: the unit normals of the float32 (V,h,w) ``depth`` maps on the GPU, in the scene frame and
    facing their cameras, from the points of neighbouring pixels (``fuse_depth_maps``' points; ``ops.depth_normals`` has the rule).
    ``mask`` and the validity of a pixel as in ``fuse_depth_maps``; with ``edge_threshold`` a neighbour whose depth differs by more
    than ``edge_threshold`` x the pixel's depth is not differenced across.  (0, 0, 0) where no normal can be formed."""
    return ops.depth_normals(depth, _views_of(depth, extrinsics, intrinsics), mask, edge_threshold)


def normals_to_u8(normals: Tensor, camera: Optional[dict] = None) -> Tensor:
    """-> uint8, the shape of the float32 (...,3) ``normals``: the picture of a normal map, 127.5 (c + 1) rounded, c the normal in
    the frame of ``camera`` (a dict as ``harness.frame_batch`` takes it: its ``pose[:3, :3]``, camera-to-world, the camera looking
    down -z with y up, so a surface that faces the camera comes out blue) or, without a camera, the scene frame.  A zero normal is
    mid-grey (128, 128, 128)."""
    rotation = None
    if camera is not None:
        rotation = numpy.asarray(camera['pose'], dtype=numpy.float64).reshape(4, 4)[:3, :3]
    return ops.normals_to_u8(normals, rotation)


def ply_mesh_bytes(points, colours, triangles, normals=None) -> bytes:
    """A binary little-endian PLY file of N vertices as ``ply_bytes`` writes them and F faces: ``property list uchar int
    vertex_indices``, 13 bytes a face.  ``triangles`` (F,3) int32, a tensor (copied to the host) or numpy; F = 0 and N = 0 are valid.
    With ``normals`` (N,3) float32 the vertex element is ``x y z nx ny nz red green blue``, 27 bytes a vertex; without, the file is
    what it was before normals existed."""
    if isinstance(triangles, torch.Tensor):
        triangles = triangles.detach().cpu().numpy()
    triangles = numpy.asarray(triangles)
    if triangles.dtype != numpy.int32 or triangles.ndim != 2 or triangles.shape[1] != 3:
        raise RuntimeError(f'triangles: expected int32 (F, 3), got {triangles.dtype} {triangles.shape}')
    vertex_file = ply_bytes(points, colours, normals)
    end = b'end_header\n'
    header, records = vertex_file.split(end, 1)
    faces = numpy.empty((triangles.shape[0],), dtype=PLY_FACE)
    faces['count'] = 3
    for a, name in enumerate(('a', 'b', 'c')):
        faces[name] = triangles[:, a]
    return (header + f'element face {triangles.shape[0]}\nproperty list uchar int vertex_indices\n'.encode('ascii') + end + records
            + faces.tobytes())


def save_ply_mesh(path, points, colours, triangles, normals=None) -> None:
    """``ply_mesh_bytes`` written to ``path``.  A file that exists is left alone, as ``save_ply`` leaves it."""
    path = os.fspath(path)
    if os.path.exists(path):
        return
    data = ply_mesh_bytes(points, colours, triangles, normals)
    os.makedirs(os.path.dirname(path) or '.', exist_ok=True)
    with open(path, 'wb') as f:
        f.write(data)
