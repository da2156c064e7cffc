"""The point-cloud export restated in plain numpy float64, pixel by pixel, in the words of simplenerf_amd/csrc/simplenerf_fuse.h
(DESIGN.md section 9 has the same rule): what tests/test_fuse_host.py pins on the CPU and tests/test_gpu_fuse.py holds the device to.
Also the analytic scene both use: two fronto-parallel planes seen by three slightly turned cameras.

Nothing here is vectorised over pixels on purpose: every step is one sentence of the rule.  The run sums of ``voxel_thin`` are
sequential Python sums (numpy.sum is pairwise and rounds differently)."""
import functools
import math

import numpy


# ---------------------------------------------------------------------------------------------------------------- the rule
def is_valid(depth, mask, v, y, x) -> bool:
    d = depth[v, y, x]
    return bool(numpy.isfinite(d) and d > 0 and (mask is None or mask[v, y, x] != 0))


def point_of(extrinsic_inverse, intrinsic_inverse, x, y, d) -> numpy.ndarray:
    """P = inv(E)[:3] . [d . inv(K) . (x, y, 1); 1]"""
    camera_point = numpy.float64(d) * numpy.matmul(intrinsic_inverse, numpy.array([x, y, 1.0]))
    return numpy.matmul(extrinsic_inverse[:3], numpy.append(camera_point, 1.0))


def fuse_depth_maps(depth, image, extrinsics, intrinsics, depth_error_threshold=0.02, min_views=1, mask=None, margins=None):
    """-> (points float32 (N,3), colours uint8 (N,3), views uint8 (N), sources int64 (N,3): the (v, y, x) of every kept pixel).
    ``margins``: a dict that receives, per valid source (v, y, x), {'tie': the smallest distance of a projection coordinate from a
    rounding tie (x.5), 'threshold': the smallest | |c_z - d_u| / d_u - tau | over its lookups, 'lookups': their number} -- how close
    each decision was (tests may leave out pixels decided within 1e-9)."""
    depth = numpy.asarray(depth, dtype=numpy.float32)
    views, h, w = depth.shape
    e = numpy.asarray(extrinsics, dtype=numpy.float64).reshape(views, 4, 4)
    k = numpy.asarray(intrinsics, dtype=numpy.float64).reshape(views, 3, 3)
    e_inv = [numpy.linalg.inv(m) for m in e]
    k_inv = [numpy.linalg.inv(m) for m in k]
    tau = float(depth_error_threshold)
    points, colours, counts, sources = [], [], [], []
    for v in range(views):
        for y in range(h):
            for x in range(w):
                if not is_valid(depth, mask, v, y, x):
                    continue
                P = point_of(e_inv[v], k_inv[v], x, y, depth[v, y, x])
                agree, tie, threshold, lookups = 0, math.inf, math.inf, 0
                for u in range(views):
                    if u == v:
                        continue
                    c = numpy.matmul(e[u, :3], numpy.append(P, 1.0))
                    if not c[2] > 0:
                        continue
                    q = numpy.matmul(k[u], c)
                    with numpy.errstate(divide='ignore', invalid='ignore', over='ignore'):
                        px, py = q[0] / q[2], q[1] / q[2]
                    ix, iy = numpy.rint(px), numpy.rint(py)               # ties to even
                    if numpy.isfinite(px) and numpy.isfinite(py):
                        tie = min(tie, abs(abs(px - math.floor(px)) - 0.5), abs(abs(py - math.floor(py)) - 0.5))
                    if not (0 <= ix < w and 0 <= iy < h):                 # (a NaN fails every comparison)
                        continue
                    if not is_valid(depth, mask, u, int(iy), int(ix)):
                        continue
                    d_u = numpy.float64(depth[u, int(iy), int(ix)])
                    lookups += 1
                    threshold = min(threshold, abs(abs(c[2] - d_u) / d_u - tau))
                    if abs(c[2] - d_u) <= tau * d_u:
                        agree += 1
                if margins is not None:
                    margins[(v, y, x)] = {'tie': tie, 'threshold': threshold, 'lookups': lookups}
                if agree >= min_views:
                    points.append(P.astype(numpy.float32))
                    colours.append(image[v, y, x])
                    counts.append(agree)
                    sources.append((v, y, x))
    return (numpy.array(points, dtype=numpy.float32).reshape(-1, 3), numpy.array(colours, dtype=numpy.uint8).reshape(-1, 3),
            numpy.array(counts, dtype=numpy.uint8), numpy.array(sources, dtype=numpy.int64).reshape(-1, 3))


def voxel_grid(points, voxel_size):
    """-> (lo float64 (3), extents (3) ints): the per-axis minimum and floor((max - lo) / voxel_size) + 1."""
    p = numpy.asarray(points, dtype=numpy.float32).astype(numpy.float64)
    lo = p.min(axis=0)
    return lo, tuple(int(math.floor((p[:, a].max() - lo[a]) / float(voxel_size))) + 1 for a in range(3))


def voxel_thin(points, colours, voxel_size):
    """-> (points float32 (M,3), colours uint8 (M,3), counts int32 (M)), runs in ascending key order."""
    points = numpy.asarray(points, dtype=numpy.float32)
    colours = numpy.asarray(colours, dtype=numpy.uint8)
    if points.shape[0] == 0:
        return points.reshape(0, 3), colours.reshape(0, 3), numpy.zeros((0,), dtype=numpy.int32)
    lo, (nx, ny, nz) = voxel_grid(points, voxel_size)
    keys = []
    for p in points:
        i = [int(math.floor((float(p[a]) - float(lo[a])) / float(voxel_size))) for a in range(3)]
        keys.append((i[2] * ny + i[1]) * nx + i[0])
    order = numpy.argsort(numpy.array(keys, dtype=numpy.int64), kind='stable')
    out_points, out_colours, out_counts = [], [], []
    at = 0
    while at < len(order):
        end = at
        while end < len(order) and keys[order[end]] == keys[order[at]]:
            end += 1
        count = end - at
        position = []
        for a in range(3):
            total = 0.0
            for j in range(at, end):                  # sequentially, in ascending source order
                total += float(points[order[j], a])
            position.append(numpy.float32(total / count))
        colour = []
        for a in range(3):
            total = 0
            for j in range(at, end):
                total += int(colours[order[j], a])
            colour.append((2 * total + count) // (2 * count))
        out_points.append(position)
        out_colours.append(colour)
        out_counts.append(count)
        at = end
    return (numpy.array(out_points, dtype=numpy.float32).reshape(-1, 3), numpy.array(out_colours, dtype=numpy.uint8).reshape(-1, 3),
            numpy.array(out_counts, dtype=numpy.int32))


def fuse_depth_maps_vectorised(scene, tau, min_views, check_margins=True):
    """The rule over whole frames (numpy float64, matmul per view pair) -> (kept bool (V,h,w), points float32 (N,3), views uint8 (N));
    ``scene``: a dict like ``scene()``'s, without a mask.  ``check_margins``: decisions within 1e-9 of a threshold or a tie are asserted
    absent.  For frames too large for the looped restatement above, to which tests hold it on the small scene first; also the host
    side of tools/measure_point_cloud.py."""
    depth, e, k = scene['depth'], scene['extrinsics'], scene['intrinsics']
    views, h, w = depth.shape
    valid = numpy.isfinite(depth) & (depth > 0)
    ys, xs = numpy.meshgrid(numpy.arange(h, dtype=numpy.float64), numpy.arange(w, dtype=numpy.float64), indexing='ij')
    pixels = numpy.stack([xs, ys, numpy.ones_like(xs)], axis=-1)
    agree = numpy.zeros(depth.shape, dtype=numpy.int64)
    points = numpy.zeros(depth.shape + (3,))
    for v in range(views):
        camera_points = depth[v].astype(numpy.float64)[..., None] * (pixels @ numpy.linalg.inv(k[v]).T)
        inverse = numpy.linalg.inv(e[v])
        points[v] = camera_points @ inverse[:3, :3].T + inverse[:3, 3]
        for u in range(views):
            if u == v:
                continue
            c = points[v] @ e[u][:3, :3].T + e[u][:3, 3]
            q = c @ k[u].T
            with numpy.errstate(divide='ignore', invalid='ignore'):
                px, py = q[..., 0] / q[..., 2], q[..., 1] / q[..., 2]
            ix, iy = numpy.rint(px), numpy.rint(py)
            inside = valid[v] & (c[..., 2] > 0) & (ix >= 0) & (ix < w) & (iy >= 0) & (iy < h)
            jx, jy = numpy.where(inside, ix, 0).astype(int), numpy.where(inside, iy, 0).astype(int)
            d_u = depth[u][jy, jx].astype(numpy.float64)
            seen = inside & valid[u][jy, jx]
            with numpy.errstate(divide='ignore', invalid='ignore'):
                error = numpy.abs(c[..., 2] - d_u) / d_u
            if check_margins:
                with numpy.errstate(invalid='ignore'):
                    ties = (numpy.abs(numpy.abs(px - numpy.floor(px)) - 0.5) < 1e-9) | (numpy.abs(numpy.abs(py - numpy.floor(py)) - 0.5) < 1e-9)
                    assert not (seen & (numpy.abs(error - tau) < 1e-9)).any() and not (inside & ties).any()
            agree[v] += seen & (numpy.abs(c[..., 2] - d_u) <= tau * d_u)
    keep = valid & (agree >= min_views)
    return keep, points[keep].astype(numpy.float32), agree[keep].astype(numpy.uint8)


# ---------------------------------------------------------------------------------------------------------------- the scene
SCENE_H, SCENE_W, SCENE_F = 13, 17, 20.0
NEAR_PLANE, FAR_PLANE, NEAR_HALF_SIDE = 5.0, 10.0, 1.3


def intrinsic_of(h, w, f):
    return numpy.array([[f, 0.0, (w - 1) / 2], [0.0, f, (h - 1) / 2], [0.0, 0.0, 1.0]])


def camera_to_world(position, yaw):
    """A camera at ``position`` looking down +z (x right, y down), turned by ``yaw`` radians about the y axis: positive yaw turns the
    optical axis towards -x (the outer cameras of the scene look towards its middle)."""
    c, s = math.cos(yaw), math.sin(yaw)
    m = numpy.eye(4)
    m[:3, :3] = [[c, 0.0, -s], [0.0, 1.0, 0.0], [s, 0.0, c]]
    m[:3, 3] = position
    return m


def plane_depths(pose, intrinsic, h, w):
    """z-depths (float64 (h,w)) of the scene from one camera: the plane z = 5 where the ray meets it inside |x|, |y| <= 1.3, else
    the plane z = 10."""
    k_inv = numpy.linalg.inv(intrinsic)
    depth = numpy.empty((h, w), dtype=numpy.float64)
    for y in range(h):
        for x in range(w):
            direction = numpy.matmul(pose[:3, :3], numpy.matmul(k_inv, numpy.array([x, y, 1.0])))     # (z-component 1 in the camera)
            t = (NEAR_PLANE - pose[2, 3]) / direction[2]
            hit = pose[:3, 3] + t * direction
            if not (abs(hit[0]) <= NEAR_HALF_SIDE and abs(hit[1]) <= NEAR_HALF_SIDE):
                t = (FAR_PLANE - pose[2, 3]) / direction[2]
            depth[y, x] = t
    return depth


def colours_of(views, h, w):
    """A colour per pixel that names it: no two neighbours alike."""
    v, y, x = numpy.meshgrid(numpy.arange(views), numpy.arange(h), numpy.arange(w), indexing='ij')
    return numpy.stack([(37 * v + 11 * y + 5 * x) % 256, (90 * v + 3 * y + 17 * x + 40) % 256, (7 * v + 29 * y + 2 * x + 128) % 256],
                       axis=-1).astype(numpy.uint8)


@functools.lru_cache(maxsize=None)
def scene(h=SCENE_H, w=SCENE_W, f=SCENE_F):
    """{'depth' float32 (3,h,w), 'image' uint8 (3,h,w,3), 'extrinsics' (3,4,4), 'intrinsics' (3,3,3), 'depth64': the depths before
    their cast to float32} of the analytic scene: three cameras at x = -1, 0, 1, y = 0, 0.1, 0.2, yaw 0.03 (i - 1) rad.  Shared
    between tests: treat it as read-only."""
    poses = [camera_to_world((i - 1.0, 0.1 * i, 0.0), 0.03 * (i - 1)) for i in range(3)]
    intrinsics = numpy.stack([intrinsic_of(h, w, f)] * 3)
    depth = numpy.stack([plane_depths(pose, intrinsics[i], h, w) for i, pose in enumerate(poses)])
    out = {'depth': depth.astype(numpy.float32), 'depth64': depth, 'image': colours_of(3, h, w), 'extrinsics': numpy.stack([numpy.linalg.inv(p) for p in poses]),
           'intrinsics': intrinsics}
    for value in out.values():
        value.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def scene_expected(depth_error_threshold, min_views):
    """The restatement on ``scene()``: (points, colours, views, sources, margins), computed once per (tau, min_views)."""
    s = scene()
    margins = {}
    result = fuse_depth_maps(s['depth'], s['image'], s['extrinsics'], s['intrinsics'], depth_error_threshold, min_views, None, margins)
    return result + (margins,)


# ---------------------------------------------------------------------------------------------------------------- native fixture
NATIVE_TAU, NATIVE_MIN_VIEWS, NATIVE_VOXEL = 0.02, 1, 0.5


def native_fixture() -> bytes:
    """What tests/native/fuse_abi_smoke.cpp reads, little-endian, in this order:
    int32 views, h, w, min_views | float64 tau | float64 cameras (views, 42) | float32 depth (views, h, w) | uint8 image (views, h, w, 3)
    | int64 N | float32 points (N, 3) | uint8 colours (N, 3) | uint8 views (N)                        the restated fuse of the scene
    | float64 voxel_size, lo (3) | int32 extents (3) | int64 M | float32 (M, 3) | uint8 (M, 3) | int32 counts (M)
                                                                                  the restated thinning of those N restated points"""
    import struct

    from simplenerf_amd import geometry
    s = scene()
    views, h, w = s['depth'].shape
    points, colours, agreeing = scene_expected(NATIVE_TAU, NATIVE_MIN_VIEWS)[:3]
    lo, extents = voxel_grid(points, NATIVE_VOXEL)
    thin_points, thin_colours, thin_counts = voxel_thin(points, colours, NATIVE_VOXEL)
    little = lambda array, dtype: numpy.ascontiguousarray(array).astype(dtype).tobytes()
    return b''.join([
        struct.pack('<4id', views, h, w, NATIVE_MIN_VIEWS, NATIVE_TAU), little(geometry.fuse_cameras(s['extrinsics'], s['intrinsics']), '<f8'),
        little(s['depth'], '<f4'), little(s['image'], 'u1'),
        struct.pack('<q', len(points)), little(points, '<f4'), little(colours, 'u1'), little(agreeing, 'u1'),
        struct.pack('<4d3iq', NATIVE_VOXEL, *lo, *extents, len(thin_points)), little(thin_points, '<f4'), little(thin_colours, 'u1'),
        little(thin_counts, '<i4')])
