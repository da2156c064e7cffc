"""The mesh export restated in plain Python / numpy float64, node by node and cell by cell, in the words of
simplenerf_amd/csrc/simplenerf_mesh.h (DESIGN.md section 9 has the same rules): what tests/test_mesh_host.py pins on the CPU and
tests/test_gpu_mesh.py holds the device to.  Also the marching-tetrahedra table generated from its sentences, the analytic scene (a
unit sphere seen by six cameras), the fixtures and the surface bookkeeping both test files use.

Nothing here is vectorised over nodes, cells or points on purpose: every step is one sentence of a rule, every sum and product is
one Python float operation in the order the header gives (Python floats are IEEE doubles; nothing is fused)."""
import functools
import itertools
import math

import numpy

AXIS_ORDERS = tuple(itertools.permutations(range(3)))            # lexicographic: xyz, xzy, yxz, yzx, zxy, zyx
EDGE_TYPES = {(1, 0, 0): 0, (0, 1, 0): 1, (0, 0, 1): 2, (1, 1, 0): 3, (1, 0, 1): 4, (0, 1, 1): 5, (1, 1, 1): 6}
OFFSET_OF_TYPE = {t: o for o, t in EDGE_TYPES.items()}
KEYS_PER_NODE = 7


# ---------------------------------------------------------------------------------------------------------------- the table
def tetrahedron(t):
    """The four vertices (offsets in the cell, (x, y, z)) of Kuhn tetrahedron ``t``: the path from the origin along axes a, b, c."""
    at = [0, 0, 0]
    path = [tuple(at)]
    for axis in AXIS_ORDERS[t]:
        at[axis] = 1
        path.append(tuple(at))
    return path


def case_triangles(t, case):
    """The triangles of tetrahedron ``t`` when bit m of ``case`` says vertex m is negative: a list of triples of edges (m, m'),
    m < m', wound so that the normal of the +-1 field's triangle looks from the negative nodes to the positive ones."""
    vertices = [numpy.array(v, dtype=numpy.float64) for v in tetrahedron(t)]
    negative = [m for m in range(4) if (case >> m) & 1]
    positive = [m for m in range(4) if not (case >> m) & 1]
    edge = lambda a, b: (min(a, b), max(a, b))
    if not negative or not positive:
        return []
    if len(negative) == 1 or len(positive) == 1:
        alone = negative[0] if len(negative) == 1 else positive[0]
        triangles = [[edge(alone, o) for o in range(4) if o != alone]]
    else:
        (n0, n1), (p0, p1) = negative, positive
        quad = [edge(n0, p0), edge(n0, p1), edge(n1, p1), edge(n1, p0)]
        triangles = [[quad[0], quad[1], quad[2]], [quad[0], quad[2], quad[3]]]
    outward = sum(vertices[m] for m in positive) / len(positive) - sum(vertices[m] for m in negative) / len(negative)
    wound = []
    for triangle in triangles:
        v0, v1, v2 = ((vertices[a] + vertices[b]) / 2 for a, b in triangle)
        if not numpy.dot(numpy.cross(v1 - v0, v2 - v0), outward) > 0:
            triangle = [triangle[0], triangle[2], triangle[1]]
            v0, v1, v2 = ((vertices[a] + vertices[b]) / 2 for a, b in triangle)
            assert numpy.dot(numpy.cross(v1 - v0, v2 - v0), outward) > 0
        wound.append(tuple(triangle))
    return wound


@functools.lru_cache(maxsize=None)
def table():
    """table()[t][case] = case_triangles(t, case), all 96."""
    return tuple(tuple(tuple(case_triangles(t, case)) for case in range(16)) for t in range(6))


# ---------------------------------------------------------------------------------------------------------------- projection
def is_valid(depth, mask, u, iy, ix) -> bool:
    d = depth[u, iy, ix]
    return bool(numpy.isfinite(d) and d > 0 and (mask is None or mask[u, iy, ix] != 0))


def _divide(a, b):
    with numpy.errstate(divide='ignore', invalid='ignore', over='ignore'):
        return float(numpy.float64(a) / numpy.float64(b))


def look_up(P, e, k, depth, mask, u):
    """Rule steps 1..4 for point ``P`` (three floats) in view ``u`` -> (c_z, d, tie, iy, ix) or None: the point's depth in the view,
    the valid depth of the pixel it lands on, the distance of the projection from a rounding tie, and that pixel."""
    E, K = e[u], k[u]
    c = [((float(E[a][0]) * P[0] + float(E[a][1]) * P[1]) + float(E[a][2]) * P[2]) + float(E[a][3]) for a in range(3)]
    if not c[2] > 0:
        return None
    q = [(float(K[a][0]) * c[0] + float(K[a][1]) * c[1]) + float(K[a][2]) * c[2] for a in range(3)]
    px, py = _divide(q[0], q[2]), _divide(q[1], q[2])
    ix, iy = float(numpy.rint(px)), float(numpy.rint(py))               # ties to even
    h, w = depth.shape[1:]
    if not (0 <= ix < w and 0 <= iy < h):                                # (a NaN fails every comparison)
        return None
    tie = min(abs(abs(px - math.floor(px)) - 0.5), abs(abs(py - math.floor(py)) - 0.5))
    if not is_valid(depth, mask, u, int(iy), int(ix)):
        return None
    return c[2], float(depth[u, int(iy), int(ix)]), tie, int(iy), int(ix)


def node_position(lo, voxel_size, index):
    return [float(lo[a]) + float(voxel_size) * index[a] for a in range(3)]


def _cameras(extrinsics, intrinsics, views):
    return (numpy.asarray(extrinsics, dtype=numpy.float64).reshape(views, 4, 4),
            numpy.asarray(intrinsics, dtype=numpy.float64).reshape(views, 3, 3))


# ---------------------------------------------------------------------------------------------------------------- integrate
def tsdf_integrate(depth, extrinsics, intrinsics, lo, voxel_size, extents, truncation, mask=None, margins=None):
    """-> (tsdf float32 (nz, ny, nx), weight uint8 (nz, ny, nx)).  ``margins``: a dict that receives 'tie' (nz, ny, nx): the smallest
    distance of a node's projections from a rounding tie, and 'behind': the smallest |s + mu| of its lookups (inf without one)."""
    depth = numpy.asarray(depth, dtype=numpy.float32)
    views = depth.shape[0]
    e, k = _cameras(extrinsics, intrinsics, views)
    nx, ny, nz = extents
    mu = float(truncation)
    tsdf = numpy.ones((nz, ny, nx), dtype=numpy.float32)
    weight = numpy.zeros((nz, ny, nx), dtype=numpy.uint8)
    ties = numpy.full((nz, ny, nx), math.inf)
    behind = numpy.full((nz, ny, nx), math.inf)
    for kk in range(nz):
        for j in range(ny):
            for i in range(nx):
                P = node_position(lo, voxel_size, (i, j, kk))
                total, count = 0.0, 0
                for u in range(views):
                    seen = look_up(P, e, k, depth, mask, u)
                    if seen is None:
                        continue
                    c_z, d, tie = seen[:3]
                    ties[kk, j, i] = min(ties[kk, j, i], tie)
                    s = d - c_z
                    behind[kk, j, i] = min(behind[kk, j, i], abs(s + mu))
                    if not s >= -mu:
                        continue
                    total += min(1.0, s / mu)
                    count += 1
                if count > 0:
                    tsdf[kk, j, i] = numpy.float32(total / count)
                weight[kk, j, i] = count
    if margins is not None:
        margins['tie'], margins['behind'] = ties, behind
    return tsdf, weight


def tsdf_integrate_vectorised(depth, extrinsics, intrinsics, lo, voxel_size, extents, truncation, slab=8):
    """The rule over whole slabs of ``slab`` z-layers (numpy float64, without a mask) -> (tsdf, weight).  Products and sums are numpy's,
    element by element in the rule's order.  For volumes too large for the looped restatement above, to which tests hold it on the
    scene first; also the host side of tools/measure_mesh.py."""
    depth = numpy.asarray(depth, dtype=numpy.float32)
    views, h, w = depth.shape
    e, k = _cameras(extrinsics, intrinsics, views)
    nx, ny, nz = extents
    mu = float(truncation)
    valid = numpy.isfinite(depth) & (depth > 0)
    tsdf = numpy.ones((nz, ny, nx), dtype=numpy.float32)
    weight = numpy.zeros((nz, ny, nx), dtype=numpy.uint8)
    x = (float(lo[0]) + float(voxel_size) * numpy.arange(nx))[None, None, :]
    y = (float(lo[1]) + float(voxel_size) * numpy.arange(ny))[None, :, None]
    for first in range(0, nz, slab):
        z = (float(lo[2]) + float(voxel_size) * numpy.arange(first, min(first + slab, nz)))[:, None, None]
        total = numpy.zeros((z.shape[0], ny, nx))
        count = numpy.zeros((z.shape[0], ny, nx), dtype=numpy.int64)
        for u in range(views):
            c = [((e[u][a][0] * x + e[u][a][1] * y) + e[u][a][2] * z) + e[u][a][3] for a in range(3)]
            q = [(k[u][a][0] * c[0] + k[u][a][1] * c[1]) + k[u][a][2] * c[2] for a in range(3)]
            with numpy.errstate(divide='ignore', invalid='ignore', over='ignore'):
                ix, iy = numpy.rint(q[0] / q[2]), numpy.rint(q[1] / q[2])
                inside = (c[2] > 0) & (ix >= 0) & (ix < w) & (iy >= 0) & (iy < h)
            jx, jy = numpy.where(inside, ix, 0).astype(numpy.int64), numpy.where(inside, iy, 0).astype(numpy.int64)
            s = depth[u][jy, jx].astype(numpy.float64) - c[2]
            with numpy.errstate(invalid='ignore'):
                used = inside & valid[u][jy, jx] & (s >= -mu)
            total += numpy.where(used, numpy.minimum(1.0, numpy.where(used, s, 0.0) / mu), 0.0)
            count += used
        seen = count > 0
        tsdf[first:first + slab][seen] = (total[seen] / count[seen]).astype(numpy.float32)
        weight[first:first + slab] = count
    return tsdf, weight


# ---------------------------------------------------------------------------------------------------------------- extract
def extract_mesh(tsdf, weight, lo, voxel_size, min_weight=1):
    """-> (vertices float32 (Nv, 3), triangles int32 (Nt, 3), keys int64 (Nv), cases: the set of (tetrahedron, case) pairs met in
    complete cells)."""
    tsdf = numpy.asarray(tsdf, dtype=numpy.float32)
    nz, ny, nx = tsdf.shape
    node = lambda i, j, k: (k * ny + j) * nx + i
    negative = lambda i, j, k: bool(tsdf[k, j, i] < 0)

    def complete(i, j, k):
        if not (0 <= i < nx - 1 and 0 <= j < ny - 1 and 0 <= k < nz - 1):
            return False
        return all(weight[k + c, j + b, i + a] >= min_weight for c in (0, 1) for b in (0, 1) for a in (0, 1))

    # the vertices, by their definition: a grid edge whose nodes differ in sign and which a complete cell contains
    keys = []
    for k in range(nz):
        for j in range(ny):
            for i in range(nx):
                for kind in range(KEYS_PER_NODE):
                    o = OFFSET_OF_TYPE[kind]
                    if i + o[0] >= nx or j + o[1] >= ny or k + o[2] >= nz:
                        continue
                    if negative(i, j, k) == negative(i + o[0], j + o[1], k + o[2]):
                        continue
                    cells = itertools.product(*[(x,) if step else (x - 1, x) for x, step in zip((i, j, k), o)])
                    if any(complete(*cell) for cell in cells):
                        keys.append(KEYS_PER_NODE * node(i, j, k) + kind)
    assert keys == sorted(keys)
    number = {key: at for at, key in enumerate(keys)}
    vertices = numpy.empty((len(keys), 3), dtype=numpy.float32)
    for at, key in enumerate(keys):
        n, kind = divmod(key, KEYS_PER_NODE)
        a = (n % nx, n // nx % ny, n // (nx * ny))
        b = tuple(x + step for x, step in zip(a, OFFSET_OF_TYPE[kind]))
        t_a, t_b = float(tsdf[a[2], a[1], a[0]]), float(tsdf[b[2], b[1], b[0]])
        s = t_a / (t_a - t_b)
        p_a, p_b = node_position(lo, voxel_size, a), node_position(lo, voxel_size, b)
        vertices[at] = [p_a[x] + s * (p_b[x] - p_a[x]) for x in range(3)]
    # the triangles
    triangles, referenced, cases = [], set(), set()
    for k in range(nz - 1):
        for j in range(ny - 1):
            for i in range(nx - 1):
                if not complete(i, j, k):
                    continue
                for t in range(6):
                    corners = [(i + o[0], j + o[1], k + o[2]) for o in tetrahedron(t)]
                    case = sum(1 << m for m in range(4) if negative(*corners[m]))
                    cases.add((t, case))
                    for triangle in table()[t][case]:
                        numbers = []
                        for m, m2 in triangle:
                            kind = EDGE_TYPES[tuple(y - x for x, y in zip(corners[m], corners[m2]))]
                            key = KEYS_PER_NODE * node(*corners[m]) + kind
                            referenced.add(key)
                            numbers.append(number[key])               # (KeyError: a reference to a vertex that does not exist)
                        triangles.append(numbers)
    assert referenced == set(keys)                                       # every vertex is referenced
    return vertices, numpy.array(triangles, dtype=numpy.int32).reshape(-1, 3), numpy.array(keys, dtype=numpy.int64), cases


# ---------------------------------------------------------------------------------------------------------------- colour
def colour_points(points, depth, image, extrinsics, intrinsics, colour_tolerance, mask=None, margins=None):
    """-> (colours uint8 (count, 3), views uint8 (count)).  ``margins``: a list that receives, per lookup, | |c_z - d| - tolerance |."""
    points = numpy.asarray(points, dtype=numpy.float32)
    depth = numpy.asarray(depth, dtype=numpy.float32)
    views = depth.shape[0]
    e, k = _cameras(extrinsics, intrinsics, views)
    colours = numpy.zeros((len(points), 3), dtype=numpy.uint8)
    agreeing = numpy.zeros((len(points),), dtype=numpy.uint8)
    for at, point in enumerate(points):
        P = [float(point[0]), float(point[1]), float(point[2])]
        total, n = [0, 0, 0], 0
        for u in range(views):
            seen = look_up(P, e, k, depth, mask, u)
            if seen is None:
                continue
            c_z, d, _, iy, ix = seen
            if margins is not None:
                margins.append(abs(abs(c_z - d) - colour_tolerance))
            if abs(c_z - d) <= colour_tolerance:
                for a in range(3):
                    total[a] += int(image[u, iy, ix, a])
                n += 1
        if n:
            colours[at] = [(2 * total[a] + n) // (2 * n) for a in range(3)]
        agreeing[at] = n
    return colours, agreeing


# ---------------------------------------------------------------------------------------------------------------- bookkeeping
def surface_statistics(vertices, triangles):
    """{'vertices', 'edges', 'faces', 'boundary_edges': undirected edges in one triangle only, 'irregular_edges': in more than two,
    'misoriented': directed edges that occur more than once, 'zero_area', 'directed': {(a, b): occurrences}}"""
    directed = {}
    for a, b, c in numpy.asarray(triangles).tolist():
        for edge in ((a, b), (b, c), (c, a)):
            directed[edge] = directed.get(edge, 0) + 1
    undirected = {}
    for (a, b), n in directed.items():
        key = (min(a, b), max(a, b))
        undirected[key] = undirected.get(key, 0) + n
    p = numpy.asarray(vertices, dtype=numpy.float64)
    t = numpy.asarray(triangles).reshape(-1, 3)
    areas = numpy.linalg.norm(numpy.cross(p[t[:, 1]] - p[t[:, 0]], p[t[:, 2]] - p[t[:, 0]]), axis=1) if len(t) else numpy.zeros((0,))
    return {'vertices': len(p), 'edges': len(undirected), 'faces': len(t),
            'boundary_edges': sum(1 for n in undirected.values() if n == 1),
            'irregular_edges': sum(1 for n in undirected.values() if n > 2),
            'misoriented': sum(1 for n in directed.values() if n > 1), 'zero_area': int((areas == 0).sum()), 'directed': directed}


def assert_closed_oriented_surface(vertices, triangles):
    """CPU test 2's properties, computed from the arrays -> the statistics."""
    s = surface_statistics(vertices, triangles)
    assert s['boundary_edges'] == 0 and s['irregular_edges'] == 0                       # every undirected edge in exactly two triangles
    assert s['misoriented'] == 0                                                        # every directed edge once ...
    assert all((b, a) in s['directed'] for a, b in s['directed'])                       # ... and its reverse once
    assert s['vertices'] - s['edges'] + s['faces'] == 2
    assert s['zero_area'] == 0
    return s


def interior_edge_violations(triangles, keys, extents):
    """-> (violations, directed edges looked at): the directed mesh edges that do not lie in an outer face of the grid and are not
    matched by exactly one opposite edge (or occur more than once themselves)."""
    nx, ny, nz = extents

    def nodes_of(key):
        n, kind = divmod(int(key), KEYS_PER_NODE)
        a = (n % nx, n // nx % ny, n // (nx * ny))
        return a, tuple(x + step for x, step in zip(a, OFFSET_OF_TYPE[kind]))

    def in_outer_face(edge):
        nodes = nodes_of(keys[edge[0]]) + nodes_of(keys[edge[1]])
        return any(all(node[axis] == side for node in nodes) for axis, n in enumerate((nx, ny, nz)) for side in (0, n - 1))

    directed = surface_statistics(numpy.zeros((len(keys), 3)), triangles)['directed']
    inner = [edge for edge in directed if not in_outer_face(edge)]
    return sum(1 for a, b in inner if directed[(a, b)] != 1 or directed.get((b, a), 0) != 1), len(inner)


# ---------------------------------------------------------------------------------------------------------------- the scene
SCENE_EYES = ((4, 0.3, 0.2), (-4, 0.25, -0.3), (0.2, 4, 0.35), (-0.3, -4, 0.15), (0.3, -0.2, 4), (0.15, 0.35, -4))
SCENE_SIZE, SCENE_F, SCENE_CENTRE, SCENE_MISS = 48, 57.97, 23.5, 8.0
GRID_EXTENTS, GRID_VOXEL, GRID_LO, GRID_MU = (25, 25, 25), 0.125, (-1.51, -1.49, -1.503), 0.5
SLAB_EXTENTS, SLAB_LO = (25, 21, 23), (-1.51, -1.24, -1.378)             # the same nodes as the cube's, fewer of them
COLOUR_TOLERANCE = 0.125


def look_at(eye):
    eye = numpy.array(eye, dtype=numpy.float64)
    z = -eye / numpy.linalg.norm(eye)
    up = numpy.array([0.0, 0.0, 1.0]) if abs(z[2]) < 0.9 else numpy.array([0.0, 1.0, 0.0])
    x = numpy.cross(z, up)
    x /= numpy.linalg.norm(x)
    y = numpy.cross(z, x)
    rotation = numpy.stack([x, y, z])
    extrinsic = numpy.eye(4)
    extrinsic[:3, :3] = rotation
    extrinsic[:3, 3] = -numpy.matmul(rotation, eye)
    return extrinsic


def sphere_view(extrinsic, intrinsic, size):
    """(depth float32 (size, size), image uint8 (size, size, 3)) of the unit sphere at the origin from one camera."""
    rotation, eye = extrinsic[:3, :3], -numpy.matmul(extrinsic[:3, :3].T, extrinsic[:3, 3])
    depth = numpy.full((size, size), SCENE_MISS, dtype=numpy.float32)
    image = numpy.zeros((size, size, 3), dtype=numpy.uint8)
    k_inv = numpy.linalg.inv(intrinsic)
    for y in range(size):
        for x in range(size):
            direction = numpy.matmul(rotation.T, numpy.matmul(k_inv, numpy.array([x, y, 1.0])))     # (z-component 1 in the camera)
            a, b, c = numpy.dot(direction, direction), 2 * numpy.dot(eye, direction), numpy.dot(eye, eye) - 1.0
            root = b * b - 4 * a * c
            if root < 0:
                continue
            t = (-b - math.sqrt(root)) / (2 * a)
            depth[y, x] = t
            image[y, x] = numpy.clip(numpy.rint(127.5 + 127.5 * (eye + t * direction)), 0, 255)
    return depth, image


@functools.lru_cache(maxsize=None)
def scene():
    """{'depth' float32 (6, 48, 48), 'image' uint8 (6, 48, 48, 3), 'extrinsics' (6, 4, 4), 'intrinsics' (6, 3, 3)}; read-only."""
    extrinsics = numpy.stack([look_at(eye) for eye in SCENE_EYES])
    intrinsic = numpy.array([[SCENE_F, 0.0, SCENE_CENTRE], [0.0, SCENE_F, SCENE_CENTRE], [0.0, 0.0, 1.0]])
    intrinsics = numpy.stack([intrinsic] * len(SCENE_EYES))
    views = [sphere_view(e, intrinsic, SCENE_SIZE) for e in extrinsics]
    out = {'depth': numpy.stack([v[0] for v in views]), 'image': numpy.stack([v[1] for v in views]), 'extrinsics': extrinsics,
           'intrinsics': intrinsics}
    for value in out.values():
        value.setflags(write=False)
    return out


def _frozen(*arrays):
    for array in arrays:
        if isinstance(array, numpy.ndarray):
            array.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def scene_volume(truncation=GRID_MU, extents=GRID_EXTENTS, lo=GRID_LO):
    """The restated integration of the scene: (tsdf, weight, margins), computed once per grid; read-only."""
    s = scene()
    margins = {}
    tsdf, weight = tsdf_integrate(s['depth'], s['extrinsics'], s['intrinsics'], lo, GRID_VOXEL, extents, truncation, None, margins)
    return _frozen(tsdf, weight) + (margins,)


@functools.lru_cache(maxsize=None)
def scene_mesh(truncation=GRID_MU, min_weight=1, extents=GRID_EXTENTS, lo=GRID_LO):
    """The restated extraction of ``scene_volume``: (vertices, triangles, keys, cases); read-only."""
    tsdf, weight, _ = scene_volume(truncation, extents, lo)
    return _frozen(*extract_mesh(tsdf, weight, lo, GRID_VOXEL, min_weight))


@functools.lru_cache(maxsize=None)
def scene_colours():
    """The restated colouring of ``scene_mesh()``'s vertices at COLOUR_TOLERANCE: (colours, views, margins)."""
    s = scene()
    margins = []
    colours, views = colour_points(scene_mesh()[0], s['depth'], s['image'], s['extrinsics'], s['intrinsics'], COLOUR_TOLERANCE, None, margins)
    return _frozen(colours, views) + (margins,)


# ---------------------------------------------------------------------------------------------------------------- other fixtures
FIELD_EXTENTS, FIELD_SEED = (7, 6, 5), 0


@functools.lru_cache(maxsize=None)
def random_field(holes=False, seed=FIELD_SEED):
    """(tsdf float32 (5, 6, 7) uniform in (-1, 1), weight uint8: all 1, or with ``holes`` about 15 % of them 0); read-only."""
    rng = numpy.random.default_rng(seed)
    nx, ny, nz = FIELD_EXTENTS
    tsdf = rng.uniform(-1.0, 1.0, (nz, ny, nx)).astype(numpy.float32)
    weight = numpy.ones((nz, ny, nx), dtype=numpy.uint8)
    if holes:
        weight[numpy.random.default_rng(seed + 1000).uniform(size=weight.shape) < 0.15] = 0
    return _frozen(tsdf, weight)


PLANE_EXTENTS = (6, 5, 4)


def plane_field():
    """tsdf = (i - 3) / 4 on a 6 x 5 x 4 grid, all weights 1: the surface passes through the nodes with i = 3."""
    nx, ny, nz = PLANE_EXTENTS
    tsdf = numpy.broadcast_to(((numpy.arange(nx) - 3) / 4).astype(numpy.float32), (nz, ny, nx)).copy()
    return tsdf, numpy.ones((nz, ny, nx), dtype=numpy.uint8)


def native_fixture() -> bytes:
    """What tests/native/mesh_abi_smoke.cpp reads, little-endian, in this order:
    int32 views, h, w, nx, ny, nz, min_weight | float64 voxel_size, lo (3), truncation, colour_tolerance | float64 cameras (views, 42)
    | float32 depth (views, h, w) | uint8 image (views, h, w, 3) | float32 tsdf (nz, ny, nx) | uint8 weight (nz, ny, nx)
    | int64 Nv, Nt | float32 vertices (Nv, 3) | int32 triangles (Nt, 3) | uint8 colours (Nv, 3) | uint8 views (Nv)
    -- the restated integration of the scene, the restated mesh of that volume and the restated colours of those vertices."""
    import struct

    from simplenerf_amd import geometry
    s = scene()
    views, h, w = s['depth'].shape
    tsdf, weight, _ = scene_volume()
    vertices, triangles = scene_mesh()[:2]
    colours, agreeing, _ = scene_colours()
    little = lambda array, dtype: numpy.ascontiguousarray(array).astype(dtype).tobytes()
    return b''.join([
        struct.pack('<7i6d', views, h, w, *GRID_EXTENTS, 1, GRID_VOXEL, *GRID_LO, GRID_MU, COLOUR_TOLERANCE),
        little(geometry.fuse_cameras(s['extrinsics'], s['intrinsics']), '<f8'), little(s['depth'], '<f4'), little(s['image'], 'u1'),
        little(tsdf, '<f4'), little(weight, 'u1'), struct.pack('<2q', len(vertices), len(triangles)), little(vertices, '<f4'),
        little(triangles, '<i4'), little(colours, 'u1'), little(agreeing, 'u1')])
